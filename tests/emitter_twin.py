"""Test infrastructure: a float64 twin of the library's particle source (csrc/emitter.cpp, csrc/emitter_device.hip), independent of both.

It restates, in numpy,
  * the generator: PCG32 (XSH-RR 64/32) with the emitter's seeding, positioned at any draw by the LCG jump-ahead;
  * the schedule: which birth indices are alive after every step (f32, operation by operation: `life -= dt` per cohort of particles born
    in the same step, retire from the front while not life > 0, then acc / owed / room);
  * the closed form: position = pos0 + vel * age in float64 from the exact uniforms, life = lifetime - age, rotation at birth = 360 * w in f32.

`bound_B` is the per-coordinate bound a float32 emitter may differ from the closed form by after `s` steps of life:
(16 + s) * 2^-23 * (cone_radius + |speed| * lifetime) -- a few ulp of the cloud's extent from two trig calls and their product on either side,
plus at most one ulp per `pos += vel * dt`.
"""
import math

import numpy as np

MULT = np.array([6364136223846793005], dtype=np.uint64)
INC = np.array([((0xda3e39cb94b95bdb << 1) | 1) & (2**64 - 1)], dtype=np.uint64)
ONE = np.array([1], dtype=np.uint64)


def pcg_advance(state, delta):
    """The state(s) `delta` draws after `state`: the affine map s -> s * MULT + INC composed with itself by repeated squaring (mod 2^64)."""
    delta = np.atleast_1d(np.asarray(delta, dtype=np.uint64)).copy()
    state = np.broadcast_to(np.asarray(state, dtype=np.uint64), delta.shape)
    acc_mult = np.ones_like(delta)
    acc_plus = np.zeros_like(delta)
    cur_mult, cur_plus = MULT.copy(), INC.copy()
    while np.any(delta):
        odd = (delta & ONE).astype(bool)
        acc_mult = np.where(odd, acc_mult * cur_mult, acc_mult)
        acc_plus = np.where(odd, acc_plus * cur_mult + cur_plus, acc_plus)
        cur_plus = (cur_mult + ONE) * cur_plus
        cur_mult = cur_mult * cur_mult
        delta >>= ONE
    return acc_mult * state + acc_plus


def pcg_output(old):
    old = np.asarray(old, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    x = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)) & m32
    r = old >> np.uint64(59)
    return ((x >> r) | (x << ((np.uint64(32) - r) & np.uint64(31)))) & m32


def pcg_seeded(seed):
    """State in front of the first draw: state = 0, step, add the seed, step."""
    s = pcg_advance(np.uint64(0), 1)
    s = s + np.array([seed & (2**64 - 1)], dtype=np.uint64)
    return pcg_advance(s, 1)[0]


def uniforms_of_birth(seed, k):
    """(u, v, wrot) of birth index k (array): draws 3k, 3k + 1, 3k + 2 of the stream; each is 24 bits / 2^24, exact in float32 and float64."""
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    s0 = pcg_advance(pcg_seeded(seed), k * np.uint64(3))
    s1 = s0 * MULT + INC
    s2 = s1 * MULT + INC
    return tuple((pcg_output(s) >> np.uint64(8)).astype(np.float64) / 16777216.0 for s in (s0, s1, s2))


# (rate, lifetime, max_particles, steps, dt) of the four runs the emitters are compared on: below the cap, saturating the cap
# (rate x lifetime > max_particles), the demo scene's values, and a fast, short-lived cloud
RUNS = [(100.0, 2.5, 300, 200, 1.0 / 30.0), (100.0, 2.5, 100, 200, 1.0 / 30.0), (10.0, 6.0, 60, 400, 1.0 / 30.0), (1000.0, 1.0, 5000, 150, 1.0 / 60.0)]


def bound_B(cfg, steps_lived):
    return (16.0 + np.asarray(steps_lived, dtype=np.float64)) * 2.0**-23 * (float(cfg.cone_radius) + abs(float(cfg.speed)) * float(cfg.lifetime))


class EmitterTwin:
    """Feed it the emitter's config (abi.vp_emitter_config) and the same dt sequence; `count`, `first`, `next` follow the schedule and
    `particles()` is the closed form of the live particles, oldest first."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.seed = int(cfg.seed)
        self.rate, self.lifetime = np.float32(cfg.rate), np.float32(cfg.lifetime)
        self.max_particles = int(cfg.max_particles)
        self.acc = np.float32(0.0)
        self.first = self.next = 0
        self.cohorts = []                 # [count, f32 life, step of birth, time of birth], oldest first
        self.steps = 0
        self.time = 0.0                   # float64 sum of the f32 dts
        if cfg.reserved[0] == 1:
            for _ in range(int(math.ceil(float(cfg.lifetime) * 30.0))):
                self.step(np.float32(1.0) / np.float32(30.0))

    @property
    def count(self):
        return self.next - self.first

    def step(self, dt):
        dt = np.float32(dt)
        assert dt >= 0 and np.isfinite(dt)
        self.steps += 1
        self.time += float(dt)
        for c in self.cohorts:
            c[1] = np.float32(c[1] - dt)
        while self.cohorts and not (self.cohorts[0][1] > 0):
            self.first += self.cohorts.pop(0)[0]
        self.acc = np.float32(self.acc + np.float32(self.rate * dt))
        if not (self.acc < np.float32(16777216.0)):
            self.acc = np.float32(16777216.0)
        owed = int(self.acc)
        self.acc = np.float32(self.acc - np.float32(owed))
        n = min(owed, self.max_particles - self.count)
        if n > 0:
            self.cohorts.append([n, self.lifetime, self.steps, self.time])
            self.next += n
        return self.count

    def particles(self):
        """dict of arrays over the live particles, oldest first: position [n, 3] float64, life float64, rotation0 float32 (the rotation field
        at birth), steps_lived int, bound float64 (bound_B of each particle)."""
        c = self.cfg
        n = self.count
        k = np.arange(self.first, self.next, dtype=np.uint64)
        counts = np.array([co[0] for co in self.cohorts], dtype=np.int64)
        assert counts.sum() == n
        steps_lived = np.repeat(np.array([self.steps - co[2] for co in self.cohorts], dtype=np.int64), counts)
        age = np.repeat(np.array([self.time - co[3] for co in self.cohorts], dtype=np.float64), counts)
        if n == 0:
            u = v = w = np.zeros(0)
        else:
            u, v, w = uniforms_of_birth(self.seed, k)
        rn = np.sqrt(u)
        phi = 2.0 * math.pi * v
        tilt = math.radians(float(c.cone_angle_deg)) * rn
        r, speed = float(c.cone_radius), float(c.speed)
        pos0 = np.stack([r * rn * np.cos(phi), r * rn * np.sin(phi), np.zeros(n)], axis=1)
        vel = speed * np.stack([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)], axis=1)
        return dict(position=pos0 + vel * age[:, None], life=float(c.lifetime) - age,
                    rotation0=(np.float32(360.0) * w.astype(np.float32)).astype(np.float32), steps_lived=steps_lived,
                    bound=bound_B(c, steps_lived))
