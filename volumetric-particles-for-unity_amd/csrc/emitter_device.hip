// emitter_device.hip -- particles that never leave the GPU (include/vpfx.h "particle source"): vp_upload_particles_device takes records that
// already live in device memory, and vp_device_emitter_* is the library's particle source (emitter.cpp: same vp_emitter_config, same PCG32
// stream, the arithmetic of vp_emitter_step term by term) simulated in device memory and handed to the binning without a host round trip.
//
//   k_emitter_move   live particles: pos += vel * dt, rot_deg += angular_velocity_deg * dt, life -= dt           (emitter.cpp:116-118)
//   k_emitter_emit   thread i of a step's n births: draws 3i, 3i+1, 3i+2 after the state the host hands over     (emitter.cpp:131-141)
//   k_emitter_pack   live particles, oldest first -> canonical 32-byte records {pos.xyz, size, rot mod 360, life, lifetime, 0}
//
// No read-back per step: every particle has the same lifetime and `life -= dt` is the same f32 operation for all of them, so particles die
// oldest first and the live set is a contiguous range [first, next) of birth indices that the HOST can follow exactly (EmitSchedule: one
// f32 `life` per cohort of particles born in the same step + the acc / owed / room logic of emitter.cpp:122-127).  Birth index k lives in
// slot k mod max_particles of a ring of two float4 per slot.  The generator is positioned per thread by the O(log) LCG jump-ahead.
// Bit-exact against emitter.cpp: counts, order, life, rotation, size, startLifetime.  Positions go through the device's sqrtf / sinf / cosf
// instead of the host's: equal to a few ulp, not bit for bit (DESIGN.md "Device particle source").
#include "vpfx_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <new>

namespace {

constexpr uint64_t PCG_MULT = 6364136223846793005ULL;
constexpr uint64_t PCG_INC = (0xda3e39cb94b95bdbULL << 1u) | 1u;      // the emitter's fixed stream constant (emitter.cpp:90)

// PCG32 XSH-RR 64/32: the output of a state (emitter.cpp:29-36) ...
__host__ __device__ inline uint32_t pcg_output(uint64_t old)
{
    const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
}
__host__ __device__ inline uint64_t pcg_next(uint64_t s) { return s * PCG_MULT + PCG_INC; }
// ... and the state `delta` draws further on: the LCG's affine map composed with itself by repeated squaring
__host__ __device__ inline uint64_t pcg_advance(uint64_t state, uint64_t delta)
{
    uint64_t acc_mult = 1u, acc_plus = 0u, cur_mult = PCG_MULT, cur_plus = PCG_INC;
    while (delta > 0) {
        if (delta & 1u) { acc_mult *= cur_mult; acc_plus = acc_plus * cur_mult + cur_plus; }
        cur_plus = (cur_mult + 1u) * cur_plus;
        cur_mult *= cur_mult;
        delta >>= 1u;
    }
    return acc_mult * state + acc_plus;
}
// uniform in [0, 1): the top 24 bits, exact in f32 (emitter.cpp:38)
__host__ __device__ inline float pcg_uniform01(uint64_t s) { return (float)(pcg_output(s) >> 8) * (1.0f / 16777216.0f); }

struct EmitConsts {
    float cone, cone_radius, speed, lifetime;      // cone = cone_angle_deg in radians, rounded to f32 on the host as emitter.cpp:128 does
    float angular_velocity_deg, size;
    int cap;                                        // ring slots = max_particles
};

__device__ __forceinline__ int ring_slot(int first_slot, int j, int cap)
{
    const int s = first_slot + j;                   // first_slot < cap, j < cap
    return s >= cap ? s - cap : s;
}

// pr = {pos.xyz, rot_deg}, vl = {vel.xyz, life} per slot
__global__ __launch_bounds__(256) void
k_emitter_move(float4* __restrict__ pr, float4* __restrict__ vl, int first_slot, int n_live, float dt, EmitConsts k)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_live) return;
    const int s = ring_slot(first_slot, j, k.cap);
    float4 p = pr[s], v = vl[s];
    p.x += v.x * dt; p.y += v.y * dt; p.z += v.z * dt;
    p.w += k.angular_velocity_deg * dt;
    v.w -= dt;
    pr[s] = p;
    vl[s] = v;
}

__global__ __launch_bounds__(256) void
k_emitter_emit(float4* __restrict__ pr, float4* __restrict__ vl, int first_slot, int n_births, uint64_t state0, EmitConsts k)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_births) return;
    const uint64_t s0 = pcg_advance(state0, 3ull * (uint64_t)i), s1 = pcg_next(s0), s2 = pcg_next(s1);
    // a point of the cone's base disc (uniform by area); a point at the rim leaves along the cone's surface, the centre along the axis (+z)
    const float u = pcg_uniform01(s0), v = pcg_uniform01(s1), wrot = pcg_uniform01(s2);
    const float rn = sqrtf(u);
    const float phi = 6.283185307179586f * v;
    const float cp = cosf(phi), sp = sinf(phi);
    const float tilt = k.cone * rn;
    const float st = sinf(tilt), ct = cosf(tilt);
    const int s = ring_slot(first_slot, i, k.cap);
    pr[s] = make_float4(k.cone_radius * rn * cp, k.cone_radius * rn * sp, 0.f, 360.0f * wrot);
    vl[s] = make_float4(k.speed * (st * cp), k.speed * (st * sp), k.speed * ct, k.lifetime);
}

__global__ __launch_bounds__(256) void
k_emitter_pack(const float4* __restrict__ pr, const float4* __restrict__ vl, int first_slot, int n_live, float4* __restrict__ out, EmitConsts k)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_live) return;
    const int s = ring_slot(first_slot, j, k.cap);
    const float4 p = pr[s], v = vl[s];
    out[2 * (size_t)j] = make_float4(p.x, p.y, p.z, k.size);
    out[2 * (size_t)j + 1] = make_float4(fmodf(p.w, 360.0f), v.w, k.lifetime, 0.f);
}

// ---- the live range, followed on the host ------------------------------------------------------------------------------------------------
struct EmitCohort { int32_t count; float life; };    // the particles born in one step share their f32 `life`
struct EmitSchedule {
    float acc = 0.f;                                 // fractional particles owed by the emission rate
    int64_t first = 0, next = 0;                     // live birth indices [first, next)
    std::deque<EmitCohort> cohorts;                  // oldest first
};

// One step of the bookkeeping of vp_emitter_step (emitter.cpp:113-127): age and retire, then what the rate owes, capped by the room left.
// Returns the number of births of this step (they take the birth indices [next - n, next)).  f32 operation by operation like the host's.
int schedule_step(EmitSchedule& s, const vp_emitter_config& c, float dt)
{
    for (EmitCohort& k : s.cohorts) k.life -= dt;
    // f32 subtraction is monotonic, so an older cohort's life never exceeds a younger one's: the dead are a prefix
    while (!s.cohorts.empty() && !(s.cohorts.front().life > 0.f)) { s.first += s.cohorts.front().count; s.cohorts.pop_front(); }
    s.acc += c.rate * dt;
    if (!(s.acc < 16777216.0f)) s.acc = 16777216.0f;
    const int owed = (int)s.acc;
    s.acc -= (float)owed;
    const int room = c.max_particles - (int)(s.next - s.first);
    const int n = owed < room ? owed : room;
    if (n > 0) { s.cohorts.push_back(EmitCohort{n, c.lifetime}); s.next += n; }
    return n > 0 ? n : 0;
}

bool dt_ok(float dt) { return dt >= 0.f && std::isfinite(dt); }

// The emitter's own validation: vp_emitter_create decides (one definition; without the prewarm it allocates an empty emitter and nothing else).
// *prewarm = the reserved[0] switch.
int check_config(const vp_emitter_config* cfg, bool* prewarm)
{
    if (!cfg) return VP_ERR_BAD_ARG;
    if (cfg->reserved[0] != 0 && cfg->reserved[0] != 1) return VP_ERR_BAD_ARG;
    vp_emitter_config plain = *cfg;
    plain.reserved[0] = 0;
    vp_emitter* probe = nullptr;
    const int rc = vp_emitter_create(&plain, &probe);
    vp_emitter_destroy(probe);
    *prewarm = cfg->reserved[0] == 1;
    return rc;
}

int prewarm_steps(const vp_emitter_config& c) { return (int)std::ceil((double)c.lifetime * 30.0); }     // emitter.cpp:97

// the probe's record writer follows vp_emitter_write_particles (emitter.cpp:42-51,158-167 keeps its helpers file-local)
bool layout_ok(const vp_particle_layout* l)
{
    if (!l || l->stride < 4) return false;
    const int32_t offs[5] = {l->off_position, l->off_size, l->off_rotation, l->off_lifetime, l->off_start_lifetime};
    for (int i = 0; i < 5; ++i) {
        const int32_t bytes = i == 0 ? 12 : 4;
        if (offs[i] < 0 || offs[i] + bytes > l->stride) return false;
    }
    return true;
}

inline void put_f32(unsigned char* rec, int32_t off, float v) { std::memcpy(rec + off, &v, 4); }

// the records k_emitter_pack writes
vp_particle_layout canonical_layout()
{
    vp_particle_layout l{};
    l.stride = 32; l.off_position = 0; l.off_size = 12; l.off_rotation = 16; l.off_lifetime = 20; l.off_start_lifetime = 24;
    l.rotation_in_radians = 0;
    return l;
}

inline unsigned blocks_of(int n) { return (unsigned)((n + 255) / 256); }

}  // namespace

struct vp_device_emitter {
    vp_ctx* ctx = nullptr;            // the owning single-device context; nullptr once vp_destroy(ctx) has orphaned the emitter
    vp_emitter_config cfg{};
    EmitConsts k{};
    uint64_t state = 0;               // PCG32 state at the next birth's first draw
    EmitSchedule sched;
    float4* d_ring = nullptr;         // [2][max_particles]: {pos.xyz, rot_deg} | {vel.xyz, life}
    float4* d_pack = nullptr;         // read-back scratch of vp_device_emitter_read_particles: [2 x pack_cap]
    int pack_cap = 0;

    float4* pr() const { return d_ring; }
    float4* vl() const { return d_ring + cfg.max_particles; }
    int live() const { return (int)(sched.next - sched.first); }
    int first_slot() const { return cfg.max_particles > 0 ? (int)(sched.first % cfg.max_particles) : 0; }
};

namespace {

// queue one step on the context's stream: move and age the survivors, then emit (a particle is not moved in the step it is born in)
int emitter_step(vp_device_emitter* e, float dt)
{
    vp_ctx* c = e->ctx;
    int n = 0;
    try { n = schedule_step(e->sched, e->cfg, dt); } catch (...) { return vp_fail(c, VP_ERR_OOM, "vp_device_emitter_step: host allocation failed"); }
    const int n_old = e->live() - n;
    if (n_old > 0) {
        hipLaunchKernelGGL(k_emitter_move, dim3(blocks_of(n_old)), dim3(256), 0, c->stream, e->pr(), e->vl(), e->first_slot(), n_old, dt, e->k);
        VP_HIP(hipGetLastError());
    }
    if (n > 0) {
        const int birth_slot = (int)((e->sched.next - n) % e->cfg.max_particles);
        hipLaunchKernelGGL(k_emitter_emit, dim3(blocks_of(n)), dim3(256), 0, c->stream, e->pr(), e->vl(), birth_slot, n, e->state, e->k);
        VP_HIP(hipGetLastError());
        e->state = pcg_advance(e->state, 3ull * (uint64_t)n);
    }
    return VP_OK;
}

int emitter_pack(vp_device_emitter* e, int n, float4* d_out)
{
    vp_ctx* c = e->ctx;
    if (n <= 0) return VP_OK;
    hipLaunchKernelGGL(k_emitter_pack, dim3(blocks_of(n)), dim3(256), 0, c->stream, e->pr(), e->vl(), e->first_slot(), n, d_out, e->k);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int pack_into_raw(vp_ctx* c, void* user)
{
    vp_device_emitter* e = static_cast<vp_device_emitter*>(user);
    return emitter_pack(e, e->live(), reinterpret_cast<float4*>(c->d_raw));
}

void free_device_arrays(vp_device_emitter* e)
{
    if (e->d_ring) (void)hipFree(e->d_ring);
    if (e->d_pack) (void)hipFree(e->d_pack);
    e->d_ring = e->d_pack = nullptr;
    e->pack_cap = 0;
}

}  // namespace

void device_emitters_orphan_all(vp_ctx* c)
{
    for (vp_device_emitter* e : c->emitters) { free_device_arrays(e); e->ctx = nullptr; }
    c->emitters.clear();
}

VP_EXPORT int vp_upload_particles_device(vp_ctx* c, const void* d_particles, int32_t count, const vp_particle_layout* lay,
                                         const float psys_local_to_world[16])
{
    if (!c) return VP_ERR_BAD_ARG;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_upload_particles_device: not available on a fan-out (multi-GPU) context");
    if (count > 0) {
        if (!d_particles || !lay || lay->stride < 4) return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: null pointer / bad layout");
        VP_HIP(hipSetDevice(c->device));
        // the pointer is looked at before anything is queued: host memory or another device's memory never reaches a copy or a kernel
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, d_particles) != hipSuccess) {
            (void)hipGetLastError();
            return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: %p is not memory the HIP runtime knows (host memory goes through vp_upload_particles)", d_particles);
        }
        const bool managed = at.type == hipMemoryTypeManaged || at.isManaged;
        if (!managed && at.type != hipMemoryTypeDevice)
            return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: %p is host memory (vp_upload_particles takes it)", d_particles);
        if (!managed && at.device != c->device)
            return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: %p belongs to device %d, the context to device %d", d_particles, at.device, c->device);
        if (!managed) {
            // ... and the records must lie inside the allocation the pointer belongs to
            hipDeviceptr_t base = nullptr; size_t size = 0;
            if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)d_particles) != hipSuccess) {
                (void)hipGetLastError();
                return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: %p belongs to no allocation the HIP runtime can name", d_particles);
            }
            const size_t off = (size_t)((const char*)d_particles - (const char*)base);
            if (off > size || (size_t)count * (size_t)lay->stride > size - off)
                return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_device: %d records of %d bytes run past the end of the allocation", count, lay->stride);
        }
    }
    UploadSource src;
    src.device = d_particles;
    return api_upload_particles_from(c, src, count, lay, psys_local_to_world, false);
}

VP_EXPORT int vp_device_emitter_create(vp_ctx* c, const vp_emitter_config* cfg, vp_device_emitter** out)
{
    if (!c) return VP_ERR_BAD_ARG;
    if (!out) return vp_fail(c, VP_ERR_BAD_ARG, "vp_device_emitter_create: null argument");
    *out = nullptr;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_device_emitter_create: not available on a fan-out (multi-GPU) context");
    bool prewarm = false;
    if (check_config(cfg, &prewarm) != VP_OK) return vp_fail(c, VP_ERR_BAD_ARG, "vp_device_emitter_create: bad vp_emitter_config (the rules of vp_emitter_create)");
    vp_device_emitter* e = new (std::nothrow) vp_device_emitter();
    if (!e) return vp_fail(c, VP_ERR_OOM, "vp_device_emitter_create: host allocation failed");
    e->ctx = c;
    e->cfg = *cfg;
    e->k.cone = cfg->cone_angle_deg * 0.017453292519943295f;
    e->k.cone_radius = cfg->cone_radius; e->k.speed = cfg->speed; e->k.lifetime = cfg->lifetime;
    e->k.angular_velocity_deg = cfg->angular_velocity_deg; e->k.size = cfg->size;
    e->k.cap = cfg->max_particles;
    // PCG32 seeding (emitter.cpp:88-93): state = 0, step, add the seed, step
    e->state = pcg_next(pcg_next(0u) + cfg->seed);
    auto fail = [&](int code) { free_device_arrays(e); delete e; return code; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(vp_fail(c, VP_ERR_HIP, "hipSetDevice failed"));
    if (cfg->max_particles > 0) {
        const hipError_t err = hipMalloc((void**)&e->d_ring, (size_t)2 * cfg->max_particles * sizeof(float4));
        if (err != hipSuccess) { e->d_ring = nullptr; return fail(vp_fail(c, err == hipErrorOutOfMemory ? VP_ERR_OOM : VP_ERR_HIP, "vp_device_emitter_create: hipMalloc failed: %s", hipGetErrorString(err))); }
    }
    try { c->emitters.push_back(e); } catch (...) { return fail(vp_fail(c, VP_ERR_OOM, "vp_device_emitter_create: host allocation failed")); }
    if (prewarm) {
        // the reference's system starts in steady state (scene:2269): one lifetime in 1/30 s steps, queued on the device
        const int steps = prewarm_steps(*cfg);
        for (int i = 0; i < steps; ++i) {
            const int rc = emitter_step(e, 1.0f / 30.0f);
            if (rc) { c->emitters.pop_back(); (void)hipStreamSynchronize(c->stream); return fail(rc); }
        }
    }
    *out = e;
    return VP_OK;
}

VP_EXPORT void vp_device_emitter_destroy(vp_device_emitter* e)
{
    if (!e) return;
    if (vp_ctx* c = e->ctx) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);                 // kernels of the emitter may still be queued
        free_device_arrays(e);
        c->emitters.erase(std::remove(c->emitters.begin(), c->emitters.end(), e), c->emitters.end());
    }
    delete e;
}

VP_EXPORT int vp_device_emitter_step(vp_device_emitter* e, float dt)
{
    if (!e) return VP_ERR_BAD_ARG;
    vp_ctx* c = e->ctx;
    if (!c) return VP_ERR_STATE;
    if (!dt_ok(dt)) return vp_fail(c, VP_ERR_BAD_ARG, "vp_device_emitter_step: dt %g", (double)dt);
    VP_HIP(hipSetDevice(c->device));
    const int rc = emitter_step(e, dt);
    return rc ? rc : e->live();
}

VP_EXPORT int vp_device_emitter_count(const vp_device_emitter* e)
{
    if (!e) return VP_ERR_BAD_ARG;
    if (!e->ctx) return VP_ERR_STATE;
    return e->live();
}

VP_EXPORT int vp_device_emitter_read_particles(vp_device_emitter* e, void* particles_out, int32_t capacity, const vp_particle_layout* layout)
{
    if (!e) return VP_ERR_BAD_ARG;
    vp_ctx* c = e->ctx;
    if (!c) return VP_ERR_STATE;
    if (capacity < 0 || (capacity > 0 && !particles_out) || !layout_ok(layout)) return vp_fail(c, VP_ERR_BAD_ARG, "vp_device_emitter_read_particles: bad buffer / layout");
    const int n = e->live() < capacity ? e->live() : capacity;
    if (n == 0) return 0;
    VP_HIP(hipSetDevice(c->device));
    if (n > e->pack_cap) {
        if (e->d_pack) VP_HIP(hipFree(e->d_pack));
        e->d_pack = nullptr; e->pack_cap = 0;
        const int cap = n + n / 4 + 64;
        VP_HIP(hipMalloc((void**)&e->d_pack, (size_t)cap * 2 * sizeof(float4)));
        e->pack_cap = cap;
    }
    int rc = emitter_pack(e, n, e->d_pack); if (rc) return rc;
    float* h = static_cast<float*>(malloc((size_t)n * 32));
    if (!h) return vp_fail(c, VP_ERR_OOM, "host allocation failed");
    hipError_t err = hipMemcpyAsync(h, e->d_pack, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) { free(h); return vp_fail(c, VP_ERR_HIP, "vp_device_emitter_read_particles: %s", hipGetErrorString(err)); }
    // the caller's layout, written as vp_emitter_write_particles writes it (emitter.cpp:158-167)
    unsigned char* rec = static_cast<unsigned char*>(particles_out);
    for (int i = 0; i < n; ++i, rec += layout->stride) {
        const float* p = h + 8 * (size_t)i;
        std::memset(rec, 0, (size_t)layout->stride);
        put_f32(rec, layout->off_position, p[0]); put_f32(rec, layout->off_position + 4, p[1]); put_f32(rec, layout->off_position + 8, p[2]);
        put_f32(rec, layout->off_size, p[3]);
        put_f32(rec, layout->off_rotation, layout->rotation_in_radians ? p[4] * 0.017453292519943295f : p[4]);
        put_f32(rec, layout->off_lifetime, p[5]);
        put_f32(rec, layout->off_start_lifetime, p[6]);
    }
    free(h);
    return n;
}

VP_EXPORT int vp_upload_particles_from_emitter(vp_ctx* c, vp_device_emitter* e, const float psys_local_to_world[16])
{
    if (!c) return VP_ERR_BAD_ARG;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_upload_particles_from_emitter: not available on a fan-out (multi-GPU) context");
    if (!e) return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_from_emitter: null emitter");
    if (!e->ctx) return vp_fail(c, VP_ERR_STATE, "vp_upload_particles_from_emitter: the emitter's context has been destroyed");
    if (e->ctx != c) return vp_fail(c, VP_ERR_BAD_ARG, "vp_upload_particles_from_emitter: the emitter belongs to another context");
    const vp_particle_layout lay = canonical_layout();
    UploadSource src;
    src.produce = pack_into_raw;
    src.user = e;
    return api_upload_particles_from(c, src, e->live(), &lay, psys_local_to_world, false);
}

VP_EXPORT int vp_emitter_schedule(const vp_emitter_config* cfg, const float* dts, int32_t n_steps, int64_t* first_out, int64_t* next_out)
{
    bool prewarm = false;
    if (check_config(cfg, &prewarm) != VP_OK || n_steps < 0 || (n_steps > 0 && (!dts || !first_out || !next_out))) return VP_ERR_BAD_ARG;
    for (int32_t i = 0; i < n_steps; ++i) if (!dt_ok(dts[i])) return VP_ERR_BAD_ARG;
    EmitSchedule s;
    try {
        if (prewarm) for (int i = 0, steps = prewarm_steps(*cfg); i < steps; ++i) schedule_step(s, *cfg, 1.0f / 30.0f);
        for (int32_t i = 0; i < n_steps; ++i) {
            schedule_step(s, *cfg, dts[i]);
            first_out[i] = s.first; next_out[i] = s.next;
        }
    } catch (...) { return VP_ERR_OOM; }
    return VP_OK;
}
