// MetavoxelManager.cs -- the reference-side binding: a Unity C# component that keeps the entry points of
// MetavoxelEngine.VolumetricParticleRenderer (Assets/Main Scene/VolumetricParticleRenderer.cs) for the hot path and
// forwards them to libvpfx through P/Invoke (include/vpfx.h).
//
// SOURCE ONLY: this container has no C# toolchain (no mono / mcs / dotnet) and Unity is closed source, so this file
// is not compiled or tested here; tests exercise the identical call sequence through the Python mirror
// (volumetric-particles-for-unity_amd/manager.py) over the same C ABI.
//
// What it replaces in the reference (nothing else of the component changes):
//   BinParticlesToMetavoxels()   VPR.cs:397-457   -> vp_bin
//   FillMetavoxels()             VPR.cs:495-520   -> vp_fill   (no per-MV ComputeBuffer / Blit any more)
//   FillMetavoxel(xx,yy,zz)      VPR.cs:559-609   -> vp_fill_metavoxel (after FillMetavoxelsBegin = vp_fill_begin)
//   RenderMetavoxels()           VPR.cs:637-713   -> vp_raymarch (no per-MV DrawMeshNow / ROP blend)
//   RenderMetavoxel(xx,yy,zz,i)  VPR.cs:766-794   -> vp_render_metavoxel (one metavoxel blended into the library's particlesRT)
//   UpdateMetavoxelPositions()   VPR.cs:370-394   -> vp_set_frame
// and what it keeps of the reference's frame around them (VPR.cs:168-220), so that the component is a drop-in for the whole callback pair:
//   OnPreRender                  VPR.cs:168-177   clear mainSceneRT, retarget the camera to it (particlesRT: cleared by vp_raymarch itself)
//   light depth map              VPR.cs:184, 320-367 -> SyncOccluders (vp_set_occluders2: the library renders the map inside vp_fill), or the
//                                                    light camera's depth read back and passed as vp_fill_params.light_depth_map
//   ZTest vs the scene depth     VPR.cs:204       -> the same solids (the library renders the eye depth), or _CameraDepthTexture read back
//                                                    and passed as vp_raymarch_params.scene_depth
//   composite + present          VPR.cs:210-219   -> Graphics.Blit(particlesTex, mainSceneRT, matBlendParticles); Blit to the back buffer
// and what it adds: the volume's shadow on the opaque scene (castVolumeShadows) -- the projection of lightPropogationTex the reference planned
// (FillVolume.shader:224-250) and never made: vp_volume_shadow_image, multiplied into mainSceneRT in front of the composite.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using UnityEngine;

namespace MetavoxelEngine
{
    // ABI 6 (additive): result records of the particle queries.  vp_particle_bounds is the name of the record AND of the function in the
    // header, so the two records the class imports a function for live here, outside the class that declares the imports.
    [StructLayout(LayoutKind.Sequential)]
    struct vp_particle_bounds              // boxes of the resident particles in a rigid frame (64 bytes)
    {
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] center_min;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] center_max;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] sphere_min;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] sphere_max;
        public float max_radius; public int counted, skipped, reserved;
    }
    [StructLayout(LayoutKind.Sequential)]
    struct vp_grid_fit                     // the grid centre that holds a light-space box (64 bytes)
    {
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] grid_center;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] ls_center;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] box_min;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] box_max;
        public float min_mv_scale; public int fits, clipped, reserved;
    }

    [RequireComponent(typeof(Camera))]
    public class MetavoxelManager : MonoBehaviour
    {
        // ---- inspector fields: same names as VolumetricParticleRenderer (VPR.cs:72-101) -----------------
        public Light dirLight;
        public ParticleSystem particleSys;
        public Cubemap displacementTexture;
        public GameObject gridCenter;
        public int numMetavoxelsX = 10, numMetavoxelsY = 10, numMetavoxelsZ = 10;
        public Vector3 mvScale = new Vector3(3, 3, 3);
        public int numVoxelsInMetavoxel = 32;
        public int numBorderVoxels = 1;
        public int updateInterval = 2;
        public int rayMarchSteps = 64;
        public Vector3 ambientColor = new Vector3(0.2f, 0.2f, 0.2f);
        public float fDisplacementScale = 0.7f;
        public bool fadeOutParticles = false;
        public float opacityFactor = 0.04f;
        public int softParticleStepDistance = 20;
        public Material matBlendParticles;         // VPR.cs:77: the reference's CompositeParticles material (Blend One OneMinusSrcAlpha, One One)
        public Shader generateLightDepthMapShader; // VPR.cs:79 (used with OccluderSource.UnityDepthTextures only)
        // ---- added by this binding ---------------------------------------------------------------------------
        public enum OccluderSource
        {
            None,                // no scene occlusion: light depth 1.0 everywhere, no ZTest (the synthetic benchmark configs)
            SceneMeshes,         // every enabled MeshRenderer on the Default layer (lightCamera.cullingMask, VPR.cs:346) whose mesh is Unity's
                                 // Cube / Cylinder / Sphere goes to the library as an analytic solid (vp_set_occluders2); the library renders
                                 // BOTH depth inputs on the GPU -- nothing is read back from Unity.  The reference's scene is 4 cubes + 4 cylinders
            UnityDepthTextures,  // the reference's own way: lightCamera.RenderWithShader (VPR.cs:184) and the main camera's depth texture
                                 // (VPR.cs:152, 204), both read back through `copyDepthMaterial` and passed as pointers
            AllSceneMeshes       // SceneMeshes' primitives as analytic solids, and EVERY other Default-layer MeshFilter as a triangle mesh
                                 // (vp_set_occluder_meshes once per distinct sharedMesh set, vp_set_occluder_instances with each renderer's
                                 // localToWorldMatrix when something moved): any mesh shadows the volume and rejects samples, nothing is read back.
                                 // The meshes must be readable (Read/Write enabled in the import settings)
        }
        public OccluderSource occluderSource = OccluderSource.SceneMeshes;
        public Material copyDepthMaterial;         // UnityDepthTextures: csharp/VpfxCopyDepth.shader (pass 0: raw depth, pass 1: linear eye depth)
        public int[] gpuDevices = new int[0];      // HIP ordinals; empty / one entry = one GPU.  N entries: the library cuts the grid into N
                                                   // light-axis slabs, one per GPU, with RCCL inside (vp_config.num_devices / devices[])
        public int rebalanceInterval = 240;        // multi-GPU: frames between vp_rebalance calls (0 = never re-cut the slabs)
        public bool asyncReadback = false;         // vp_raymarch_async: the image is shown one frame late, its copy runs beside the next frame's fill
        public bool useRenderThread = false;       // run the frame from Unity's render thread (GL.IssuePluginEvent) instead of OnPostRender
        public bool castVolumeShadows = false;     // CompositeParticles darkens mainSceneRT by the volume's shadow (vp_volume_shadow_image) before the blend
        public float shadowStrength = 1.0f;        // vp_shadow_params.strength: 0 = none .. 1 = the light-propagation map's value
        public int shadowFilter = 1;               // VP_SHADOW_NEAREST = 0, VP_SHADOW_BILINEAR = 1
        public Material matMultiplyShadow;         // csharp/VpfxMultiplyShadow.shader (Blend DstColor Zero, ColorMask RGB)

        // ---- C ABI (include/vpfx.h) ---------------------------------------------------------------------
        [StructLayout(LayoutKind.Sequential)]
        struct vp_config
        {
            public int nx, ny, nz, num_voxels, num_border; public float mv_scale;
            public int width, height, device, slab_z0, slab_z1, exact_math, no_early_out;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public int[] reserved;
            // ABI 3: multi-GPU fan-out inside the library
            public int num_devices;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 8)] public int[] devices;
            public int world_size, first_rank, multi_flags, rm_groups;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 128)] public byte[] rccl_unique_id;
        }
        [StructLayout(LayoutKind.Sequential)]
        struct vp_particle_layout
        {
            public int stride, off_position, off_size, off_rotation, off_lifetime, off_start_lifetime, rotation_in_radians, reserved;
        }
        [StructLayout(LayoutKind.Sequential)]
        struct vp_fill_params
        {
            public float opacity_factor, displacement_scale; public int fade_out_particles;
            public float ambient_r, ambient_g, ambient_b, init_light_intensity, light_near, light_far, light_cam_distance;
            public int cubemap_size, cubemap_format;   // VP_CUBEMAP_F32 = 0, VP_CUBEMAP_R8 = 1
            public IntPtr cubemap, light_depth_map;
        }
        [StructLayout(LayoutKind.Sequential)]
        struct vp_camera
        {
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public float[] world_to_camera;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public float[] camera_to_world;
            public float px, py, pz, fov_y, near_clip, far_clip;
        }
        [StructLayout(LayoutKind.Sequential)]
        struct vp_raymarch_params
        {
            public int steps_per_mv, soft_distance; public IntPtr scene_depth;
            public int flags;      // VP_RM_* bits (1 = UNORM8 render-target emulation, 2 / 4 / 8 = debug views; 8 = _ShowMetavoxelDrawOrder)
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public int[] reserved;
        }

        [StructLayout(LayoutKind.Sequential)]
        struct vp_occluder                     // ABI 6: typed occluder solid (0 box, 1 capped cylinder about its local y, 2 ellipsoid)
        {
            public float cx, cy, cz;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 9)] public float[] axes;
            public float hx, hy, hz;
            public int type;
        }

        [StructLayout(LayoutKind.Sequential)]
        struct vp_mesh                         // ABI 6 (additive): one occluder shape in object space; IntPtr fields over pinned arrays
        {
            public IntPtr positions, indices;  // float[n_vertices * 3], int[n_triangles * 3] (Mesh.vertices / Mesh.triangles)
            public int n_vertices, n_triangles;
        }

        [StructLayout(LayoutKind.Sequential)]
        struct vp_mesh_instance                // ABI 6 (additive): one renderer placing a shape (80 bytes)
        {
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public float[] object_to_world;
            public int mesh;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public int[] reserved;
        }

        [StructLayout(LayoutKind.Sequential)]
        struct vp_shadow_params                // ABI 6 (additive): how the light-propagation map is sampled for the volume's shadow (16 bytes)
        {
            public int filter; public float strength;
            public int reserved0, reserved1;   // must be 0
        }

        [StructLayout(LayoutKind.Sequential)]
        struct vp_unity_frame                  // one frame for the render-thread callback (include/vpfx.h "Unity native-plugin hookup")
        {
            public IntPtr ctx; public int flags, particle_count;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public float[] light_to_world;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 3)] public float[] grid_center;
            [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public float[] psys_local_to_world;
            public IntPtr particles;
            public vp_particle_layout layout; public vp_fill_params fill; public vp_camera camera; public vp_raymarch_params raymarch;
        }

        const string LIB = "vpfx";
        [DllImport(LIB)] static extern int vp_create(ref vp_config cfg, out IntPtr ctx);
        [DllImport(LIB)] static extern void vp_destroy(IntPtr ctx);
        [DllImport(LIB)] static extern IntPtr vp_last_error(IntPtr ctx);
        [DllImport(LIB)] static extern int vp_set_frame(IntPtr ctx, float[] lightToWorld, float[] gridCenter);
        [DllImport(LIB)] static extern int vp_bin(IntPtr ctx, IntPtr particles, int count, ref vp_particle_layout layout, float[] psysLocalToWorld);
        [DllImport(LIB)] static extern int vp_fill(IntPtr ctx, ref vp_fill_params p);
        [DllImport(LIB)] static extern int vp_fill_begin(IntPtr ctx, ref vp_fill_params p);
        [DllImport(LIB)] static extern int vp_fill_metavoxel(IntPtr ctx, int xx, int yy, int zz);
        [DllImport(LIB)] static extern int vp_raymarch(IntPtr ctx, ref vp_camera cam, ref vp_raymarch_params p, IntPtr rgbaOut);
        [DllImport(LIB)] static extern int vp_raymarch_async(IntPtr ctx, ref vp_camera cam, ref vp_raymarch_params p, IntPtr rgbaOut);   // image lands by vp_wait_image
        [DllImport(LIB)] static extern int vp_wait_image(IntPtr ctx);
        [DllImport(LIB)] static extern int vp_clear_particles_rt(IntPtr ctx);
        [DllImport(LIB)] static extern int vp_render_metavoxel(IntPtr ctx, ref vp_camera cam, ref vp_raymarch_params p, int xx, int yy, int zz,
                                                               int blendOver, int orderIndex);
        [DllImport(LIB)] static extern int vp_read_particles_rt(IntPtr ctx, IntPtr rgbaOut);
        [DllImport(LIB)] static extern int vp_pin_host_buffer(IntPtr ctx, IntPtr ptr, ulong bytes);
        [DllImport(LIB)] static extern int vp_unpin_host_buffer(IntPtr ctx, IntPtr ptr);
        [DllImport(LIB)] static extern int vp_rebalance(IntPtr ctx);
        [DllImport(LIB)] static extern int vp_set_occluders2(IntPtr ctx, IntPtr solids, int n);   // IntPtr: an array of vp_occluder marshalled by hand (ByValArray members)
        [DllImport(LIB)] static extern int vp_set_occluder_meshes(IntPtr ctx, vp_mesh[] meshes, int n);
        [DllImport(LIB)] static extern int vp_set_occluder_instances(IntPtr ctx, IntPtr instances, int n);   // IntPtr: vp_mesh_instance[] marshalled by hand
        [DllImport(LIB)] static extern IntPtr vp_unity_render_event_func();
        [DllImport(LIB)] static extern int vp_unity_set_frame_desc(int slot, ref vp_unity_frame frame);
        [DllImport(LIB)] static extern int vp_unity_register_output(int slot, IntPtr dRgbaOut, IntPtr hRgbaOut);
        [DllImport(LIB)] static extern int vp_unity_last_status(int slot, out ulong eventsRun);
        [DllImport(LIB)] static extern int vp_unity_clear_slot(int slot);
        [DllImport(LIB)] static extern int vp_unity_register_output_fd(int slot, IntPtr ctx, int fd, ulong bytes, ulong offset);   // texture interop: the exported render-texture memory
        [DllImport(LIB)] static extern int vp_particle_bounds(IntPtr ctx, float[] worldToFrame, out vp_particle_bounds bounds);   // null frame = world space
        [DllImport(LIB)] static extern int vp_volume_shadow_image(IntPtr ctx, ref vp_camera cam, IntPtr sceneDepth, ref vp_shadow_params p, IntPtr shadowOut);   // sceneDepth NULL = the eye depth the library renders
        [DllImport(LIB)] static extern int vp_volume_shadow_points(IntPtr ctx, float[] worldXyz, long n, ref vp_shadow_params p, float[] factorsOut);
        [DllImport(LIB)] static extern int vp_fit_grid(float[] lightToWorld, float[] lsMin, float[] lsMax, int[] numMv, float mvScale, float snap, out vp_grid_fit fit);

        IntPtr ctx = IntPtr.Zero;
        ParticleSystem.Particle[] parts;
        byte[] cubemapR;               // .x channel of the displacement cubemap as R8 (the asset is ARGB32, 8 bits per channel:
                                       // Assets/Textures/DisplacementTexture.cubemap:10-23), faces +X,-X,+Y,-Y,+Z,-Z, row 0 = top
        bool cubemapResident = false;
        bool filledOnce = false;
        bool bShowMetavoxelDrawOrder = false;                              // VPR.cs:98
        float[] rgba;                  // particlesRT as float RGBA (premultiplied), row 0 = bottom
        GCHandle rgbaHandle;           // pinned for the component's lifetime (vp_pin_host_buffer)
        Texture2D particlesTex;
        Quaternion lightOrientation;
        Vector3 wsGridCenter;
        RenderTexture mainSceneRT;     // VPR.cs:110, 236-244: the camera draws the opaque scene into this; its depth is what the ray-march is tested against
        RenderTexture lightDepthMap;   // VPR.cs:116, 275-281 (UnityDepthTextures only)
        GameObject lightCamera;        // VPR.cs:119, 320-367 (UnityDepthTextures only)
        float[] lightDepth, sceneDepth;            // read-back copies handed to the library (UnityDepthTextures only)
        GCHandle lightDepthHandle, sceneDepthHandle;
        Texture2D lightDepthTex, sceneDepthTex;
        int occluderHash = 0; bool occludersSent = false;
        int meshShapesHash = 0; bool meshShapesSent = false;   // AllSceneMeshes: the sharedMesh list the context holds
        float[] shadow;                // castVolumeShadows: the factor image [H][W], row 0 = bottom (allocated by the first frame that needs it)
        GCHandle shadowHandle;
        Texture2D shadowTex;

        static float[] ToArray(Matrix4x4 m)   // Unity Matrix4x4 is column-major in memory: m00,m10,m20,m30,m01,...
        {
            var a = new float[16];
            for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) a[c * 4 + r] = m[r, c];
            return a;
        }

        bool Check(int rc, string what)
        {
            // the reference logs and carries on (VPR.cs:352,790); so do we
            if (rc != 0) Debug.LogError(what + " failed (" + rc + "): " + Marshal.PtrToStringAnsi(vp_last_error(ctx)));
            return rc == 0;
        }

        void Start()                                                       // VPR.cs:132-149
        {
            var cfg = new vp_config {
                nx = numMetavoxelsX, ny = numMetavoxelsY, nz = numMetavoxelsZ, num_voxels = numVoxelsInMetavoxel,
                num_border = numBorderVoxels, mv_scale = mvScale.x, width = Screen.width, height = Screen.height,
                device = -1, slab_z0 = 0, slab_z1 = 0, exact_math = 0, no_early_out = 0, reserved = new int[3],
                num_devices = gpuDevices.Length > 1 ? gpuDevices.Length : 0, devices = new int[8], world_size = 0, first_rank = 0,
                multi_flags = 0, rm_groups = 0, rccl_unique_id = new byte[128] };
            if (gpuDevices.Length == 1) cfg.device = gpuDevices[0];
            for (int i = 0; i < gpuDevices.Length && i < 8; i++) cfg.devices[i] = gpuDevices[i];    // the ONE thing a multi-GPU host adds
            int rc = vp_create(ref cfg, out ctx);
            if (rc != 0) { Debug.LogError("vp_create failed (" + rc + "): " + Marshal.PtrToStringAnsi(vp_last_error(IntPtr.Zero))); return; }
            parts = new ParticleSystem.Particle[particleSys.maxParticles];
            rgba = new float[Screen.width * Screen.height * 4];
            // the read-back target lives as long as the component: pin it once and page-lock it for DMA-speed copies
            rgbaHandle = GCHandle.Alloc(rgba, GCHandleType.Pinned);
            vp_pin_host_buffer(ctx, rgbaHandle.AddrOfPinnedObject(), (ulong)rgba.Length * 4);   // speed hint only: failure is harmless
            particlesTex = new Texture2D(Screen.width, Screen.height, TextureFormat.RGBAFloat, false);
            if (useRenderThread) vp_unity_register_output(0, IntPtr.Zero, rgbaHandle.AddrOfPinnedObject());   // slot 0: particlesRT read back to `rgba`
            int S = displacementTexture.width;
            cubemapR = new byte[6 * S * S];
            CubemapFace[] faces = { CubemapFace.PositiveX, CubemapFace.NegativeX, CubemapFace.PositiveY,
                                    CubemapFace.NegativeY, CubemapFace.PositiveZ, CubemapFace.NegativeZ };
            for (int f = 0; f < 6; f++)
            {
                Color[] px = displacementTexture.GetPixels(faces[f]);
                for (int i = 0; i < S * S; i++) cubemapR[f * S * S + i] = (byte)Mathf.RoundToInt(px[i].r * 255f);   // exact for an 8-bit texture
            }
            lightOrientation = dirLight.transform.rotation;
            wsGridCenter = gridCenter.transform.position;
            UpdateMetavoxelPositions();
            CreateSceneTargets();
        }

        // mainSceneRT (VPR.cs:236-244) and, for OccluderSource.UnityDepthTextures, lightDepthMap + the camera at the light (VPR.cs:275-281, 320-367)
        void CreateSceneTargets()
        {
            Camera cam = GetComponent<Camera>();
            mainSceneRT = new RenderTexture(Screen.width, Screen.height, 24, RenderTextureFormat.ARGB32);
            mainSceneRT.Create();
            cam.targetTexture = mainSceneRT;
            if (occluderSource != OccluderSource.UnityDepthTextures) return;
            cam.depthTextureMode = DepthTextureMode.Depth;                 // VPR.cs:152: _CameraDepthTexture
            int lw = numMetavoxelsX * numVoxelsInMetavoxel, lh = numMetavoxelsY * numVoxelsInMetavoxel;
            lightDepthMap = new RenderTexture(lw, lh, 24, RenderTextureFormat.Depth);
            lightDepthMap.Create();
            lightCamera = new GameObject("LightCamera");
            lightCamera.transform.parent = dirLight.transform;
            lightCamera.SetActive(false);
            Camera lc = lightCamera.AddComponent<Camera>();
            float r = numMetavoxelsX * mvScale.x * 0.5f, t = numMetavoxelsY * mvScale.y * 0.5f;
            lc.orthographic = true;
            lc.projectionMatrix = Matrix4x4.Ortho(-r, r, -t, t, 0.3f, 1000f);                  // tight fit to the grid, VPR.cs:338-342
            lc.targetTexture = lightDepthMap;
            lc.cullingMask = 1 << LayerMask.NameToLayer("Default");
            lc.clearFlags = CameraClearFlags.Depth | CameraClearFlags.Color;
            lc.useOcclusionCulling = false;
            PlaceLightCamera();
            lightDepth = new float[lw * lh]; sceneDepth = new float[Screen.width * Screen.height];
            lightDepthHandle = GCHandle.Alloc(lightDepth, GCHandleType.Pinned);
            sceneDepthHandle = GCHandle.Alloc(sceneDepth, GCHandleType.Pinned);
            lightDepthTex = new Texture2D(lw, lh, TextureFormat.RFloat, false);
            sceneDepthTex = new Texture2D(Screen.width, Screen.height, TextureFormat.RFloat, false);
        }

        void PlaceLightCamera()                                            // UpdatePositionOfCameraAtLight, VPR.cs:361-367
        {
            if (lightCamera == null) return;
            lightCamera.transform.position = wsGridCenter - dirLight.transform.forward * 200f;
            lightCamera.transform.localRotation = Quaternion.identity;
        }

        void OnPreRender()                                                 // VPR.cs:168-177
        {
            // particlesRT lives in the library: vp_raymarch starts from dst = 0 (what GL.Clear(false, true, (0,0,0,0)) does at VPR.cs:171-172);
            // the per-metavoxel path clears it with ClearParticlesRT().  mainSceneRT is Unity's: clear it and make the camera draw into it.
            if (mainSceneRT == null) return;
            RenderTexture.active = mainSceneRT;
            GL.Clear(true, true, Color.black);
            GetComponent<Camera>().targetTexture = mainSceneRT;
        }

        void OnDestroy()
        {
            if (ctx == IntPtr.Zero) return;
            // an issued render-thread event may still be pending or running: detach the slot first (waits for a running event; a later one is a
            // no-op), only then free what its frame description pointed to
            if (useRenderThread) vp_unity_clear_slot(0);
            if (rgbaHandle.IsAllocated) { vp_unpin_host_buffer(ctx, rgbaHandle.AddrOfPinnedObject()); rgbaHandle.Free(); }
            if (partsHandle.IsAllocated) partsHandle.Free();
            if (cubeHandle.IsAllocated) cubeHandle.Free();
            if (lightDepthHandle.IsAllocated) lightDepthHandle.Free();
            if (sceneDepthHandle.IsAllocated) sceneDepthHandle.Free();
            if (shadowHandle.IsAllocated) shadowHandle.Free();
            vp_destroy(ctx); ctx = IntPtr.Zero;
        }

        void OnPostRender()                                                // VPR.cs:181-220
        {
            if (ctx == IntPtr.Zero) return;
            if (useRenderThread) { IssueFrameOnRenderThread(); return; }
            if (gpuDevices.Length > 1 && rebalanceInterval > 0 && Time.frameCount % rebalanceInterval == 0) vp_rebalance(ctx);
            // the light's view of the opaque scene (VPR.cs:184): the solids themselves (the library renders the map inside vp_fill), or Unity's render read back
            SyncOccluders();
            // the very first call always bins + fills: ray-marching before any fill is VP_ERR_STATE
            if (Time.frameCount % updateInterval == 0 || !filledOnce)
            {
                if (dirLight.transform.rotation != lightOrientation || wsGridCenter != gridCenter.transform.position)
                {
                    lightOrientation = dirLight.transform.rotation;
                    wsGridCenter = gridCenter.transform.position;
                    UpdateMetavoxelPositions();
                    PlaceLightCamera();
                }
                BinParticlesToMetavoxels();
                FillMetavoxels();
            }
            // depth-tested against the opaque scene's depth (VPR.cs:204), result in particlesTex
            RenderMetavoxels();
            CompositeParticles();
        }

        // Blend the particles onto the opaque scene and present (VPR.cs:210, 216-219; CompositeParticles.shader:10 -- the reference's own material).
        // contextIdle = false: a render-thread event may be running on the context, so no library call is made (the scene keeps last frame's look).
        void CompositeParticles(bool contextIdle = true)
        {
            if (mainSceneRT == null) return;
            if (castVolumeShadows && contextIdle && filledOnce && matMultiplyShadow != null) CastVolumeShadow();
            if (matBlendParticles != null) Graphics.Blit(particlesTex, mainSceneRT, matBlendParticles);
            GetComponent<Camera>().targetTexture = null;                   // else the Blit to the back buffer does not work (VPR.cs:218)
            Graphics.Blit(mainSceneRT, null as RenderTexture);
        }

        // The other half of the effect: the opaque scene under the smoke loses the light the volume took.  The factor image comes from the light-
        // propagation map of the last fill and the same depth source as the ray-march (SceneDepthPtr: the read-back copy, or NULL = the eye depth the
        // library renders from the solids it holds); mainSceneRT.rgb is multiplied by it in front of the composite.
        void CastVolumeShadow()
        {
            if (shadow == null)
            {
                shadow = new float[Screen.width * Screen.height];
                shadowHandle = GCHandle.Alloc(shadow, GCHandleType.Pinned);
                shadowTex = new Texture2D(Screen.width, Screen.height, TextureFormat.RFloat, false);
            }
            vp_camera cam; vp_raymarch_params rp;
            CameraAndParams(out cam, out rp);
            var sp = new vp_shadow_params { filter = shadowFilter, strength = Mathf.Clamp01(shadowStrength), reserved0 = 0, reserved1 = 0 };
            if (!Check(vp_volume_shadow_image(ctx, ref cam, SceneDepthPtr(), ref sp, shadowHandle.AddrOfPinnedObject()), "vp_volume_shadow_image")) return;
            shadowTex.SetPixelData(shadow, 0);
            shadowTex.Apply(false);
            Graphics.Blit(shadowTex, mainSceneRT, matMultiplyShadow);
        }

        // The light a point in the world still gets through the volume (light probes, forward-lit objects): multiply the directional light by it.
        public float[] VolumeShadowAt(Vector3[] worldPoints)
        {
            var xyz = new float[worldPoints.Length * 3];
            for (int i = 0; i < worldPoints.Length; i++) { xyz[3 * i] = worldPoints[i].x; xyz[3 * i + 1] = worldPoints[i].y; xyz[3 * i + 2] = worldPoints[i].z; }
            var factors = new float[worldPoints.Length];
            var sp = new vp_shadow_params { filter = shadowFilter, strength = Mathf.Clamp01(shadowStrength), reserved0 = 0, reserved1 = 0 };
            if (!filledOnce || !Check(vp_volume_shadow_points(ctx, xyz, (long)worldPoints.Length, ref sp, factors), "vp_volume_shadow_points"))
                for (int i = 0; i < factors.Length; i++) factors[i] = 1.0f;
            return factors;
        }

        // The opaque scene as the library sees it.  SceneMeshes: collect the Default-layer primitives and hand them over when something moved.
        // UnityDepthTextures: render the light's depth map the reference's way (VPR.cs:184) and read both depth textures back.
        void SyncOccluders()
        {
            if (occluderSource == OccluderSource.None) return;
            if (occluderSource == OccluderSource.UnityDepthTextures) { ReadBackDepthTextures(); return; }
            var solids = new List<vp_occluder>();
            var shapes = new List<Mesh>();
            var instances = new List<vp_mesh_instance>();
            int hash = 17;
            int defaultLayer = LayerMask.NameToLayer("Default");
            foreach (MeshRenderer mr in FindObjectsOfType<MeshRenderer>())
            {
                if (!mr.enabled || mr.gameObject.layer != defaultLayer) continue;
                MeshFilter mf = mr.GetComponent<MeshFilter>();
                if (mf == null || mf.sharedMesh == null) continue;
                int type;
                string mesh = mf.sharedMesh.name;
                if (mesh == "Cube") type = 0; else if (mesh == "Cylinder") type = 1; else if (mesh == "Sphere") type = 2;
                else if (occluderSource == OccluderSource.AllSceneMeshes)
                {
                    int shape = shapes.IndexOf(mf.sharedMesh);
                    if (shape < 0) { shape = shapes.Count; shapes.Add(mf.sharedMesh); }
                    Matrix4x4 l2w = mr.localToWorldMatrix;
                    instances.Add(new vp_mesh_instance { object_to_world = ToArray(l2w), mesh = shape, reserved = new int[3] });
                    hash = hash * 31 + l2w.GetHashCode(); hash = hash * 31 + mf.sharedMesh.GetInstanceID();
                    continue;
                }
                else continue;                                             // other meshes (SceneMeshes): use OccluderSource.AllSceneMeshes or UnityDepthTextures
                Transform t = mr.transform;
                Vector3 c = t.position, sc = t.lossyScale, ax = t.right, ay = t.up, az = t.forward;
                // Unity's primitives: Cube spans [-0.5, 0.5]^3; Cylinder: radius 0.5, height 2 about local y; Sphere: radius 0.5
                var o = new vp_occluder { cx = c.x, cy = c.y, cz = c.z, axes = new float[] { ax.x, ax.y, ax.z, ay.x, ay.y, ay.z, az.x, az.y, az.z },
                                          hx = 0.5f * Mathf.Abs(sc.x), hy = (type == 1 ? 1.0f : 0.5f) * Mathf.Abs(sc.y), hz = 0.5f * Mathf.Abs(sc.z), type = type };
                solids.Add(o);
                hash = hash * 31 + c.GetHashCode(); hash = hash * 31 + t.rotation.GetHashCode(); hash = hash * 31 + sc.GetHashCode(); hash = hash * 31 + type;
            }
            if (occludersSent && hash == occluderHash) return;             // nothing moved: the solids in the context are current
            int size = Marshal.SizeOf(typeof(vp_occluder));                // 64
            IntPtr buf = Marshal.AllocHGlobal(Math.Max(1, solids.Count) * size);
            try
            {
                for (int i = 0; i < solids.Count; i++) Marshal.StructureToPtr(solids[i], new IntPtr(buf.ToInt64() + (long)i * size), false);
                bool ok = Check(vp_set_occluders2(ctx, solids.Count > 0 ? buf : IntPtr.Zero, solids.Count), "vp_set_occluders2");
                if (occluderSource == OccluderSource.AllSceneMeshes) ok = SyncOccluderMeshes(shapes, instances) && ok;
                if (ok) { occluderHash = hash; occludersSent = true; }
            }
            finally { Marshal.FreeHGlobal(buf); }
        }

        // AllSceneMeshes: the shapes (vertex data) only when the set of distinct sharedMeshes changed, the 80-byte instances whenever something moved.
        // The library copies during each call, so the pins end with it.
        bool SyncOccluderMeshes(List<Mesh> shapes, List<vp_mesh_instance> instances)
        {
            int shapesHash = 17;
            foreach (Mesh m in shapes) shapesHash = shapesHash * 31 + m.GetInstanceID();
            if (!meshShapesSent || shapesHash != meshShapesHash)
            {
                var pins = new List<GCHandle>();
                var descs = new vp_mesh[Math.Max(1, shapes.Count)];
                try
                {
                    for (int i = 0; i < shapes.Count; i++)
                    {
                        Vector3[] v = shapes[i].vertices;
                        int[] tri = shapes[i].triangles;
                        var pos = new float[v.Length * 3];
                        for (int k = 0; k < v.Length; k++) { pos[3 * k] = v[k].x; pos[3 * k + 1] = v[k].y; pos[3 * k + 2] = v[k].z; }
                        GCHandle hp = GCHandle.Alloc(pos, GCHandleType.Pinned);
                        pins.Add(hp);
                        GCHandle ht = GCHandle.Alloc(tri, GCHandleType.Pinned);
                        pins.Add(ht);
                        descs[i] = new vp_mesh { positions = hp.AddrOfPinnedObject(), indices = ht.AddrOfPinnedObject(), n_vertices = v.Length, n_triangles = tri.Length / 3 };
                    }
                    if (!Check(vp_set_occluder_meshes(ctx, descs, shapes.Count), "vp_set_occluder_meshes")) return false;
                    meshShapesHash = shapesHash; meshShapesSent = true;
                }
                finally { foreach (GCHandle h in pins) h.Free(); }
            }
            int size = Marshal.SizeOf(typeof(vp_mesh_instance));            // 80
            IntPtr buf = Marshal.AllocHGlobal(Math.Max(1, instances.Count) * size);
            try
            {
                for (int i = 0; i < instances.Count; i++) Marshal.StructureToPtr(instances[i], new IntPtr(buf.ToInt64() + (long)i * size), false);
                return Check(vp_set_occluder_instances(ctx, instances.Count > 0 ? buf : IntPtr.Zero, instances.Count), "vp_set_occluder_instances");
            }
            finally { Marshal.FreeHGlobal(buf); }
        }

        // OccluderSource.UnityDepthTextures: the two depth inputs exactly as the reference produces them, copied to host arrays.
        //   light: lightCamera.RenderWithShader(generateLightDepthMapShader) -> lightDepthMap (D3D ortho depth, VPR.cs:184; Fill.shader:217-218 reads it raw)
        //   eye:   _CameraDepthTexture -> linear eye depth (what RM.shader:14's ZTest compares after projection)
        // row 0 of both arrays = bottom row of the view (Texture2D.ReadPixels' order = the library's image order).
        void ReadBackDepthTextures()
        {
            if (lightCamera == null || copyDepthMaterial == null) return;
            lightCamera.GetComponent<Camera>().RenderWithShader(generateLightDepthMapShader, null as string);
            ReadDepth(lightDepthMap, lightDepthTex, lightDepth, 0);
            ReadDepth(null, sceneDepthTex, sceneDepth, 1);                 // pass 1 samples _CameraDepthTexture itself
        }

        void ReadDepth(RenderTexture src, Texture2D staging, float[] dst, int pass)
        {
            RenderTexture tmp = RenderTexture.GetTemporary(staging.width, staging.height, 0, RenderTextureFormat.RFloat);
            Graphics.Blit(src, tmp, copyDepthMaterial, pass);
            RenderTexture.active = tmp;
            staging.ReadPixels(new Rect(0, 0, staging.width, staging.height), 0, 0, false);
            RenderTexture.active = null;
            RenderTexture.ReleaseTemporary(tmp);
            Color[] px = staging.GetPixels();
            for (int i = 0; i < dst.Length; i++) dst[i] = px[i].r;
        }

        // what goes into vp_fill_params.light_depth_map / vp_raymarch_params.scene_depth: NULL means "the library renders it from the solids it
        // holds" (SceneMeshes) or "no occlusion" (None); with UnityDepthTextures it is the read-back copy -- never NULL once the targets exist
        IntPtr LightDepthMapPtr()
        {
            return occluderSource == OccluderSource.UnityDepthTextures && lightDepthHandle.IsAllocated ? lightDepthHandle.AddrOfPinnedObject() : IntPtr.Zero;
        }
        IntPtr SceneDepthPtr()
        {
            return occluderSource == OccluderSource.UnityDepthTextures && sceneDepthHandle.IsAllocated ? sceneDepthHandle.AddrOfPinnedObject() : IntPtr.Zero;
        }

        // The same frame from Unity's render thread: describe it, GL.IssuePluginEvent, pick the result up next frame (the callback runs
        // [vp_set_frame] -> [vp_bin -> vp_fill] -> vp_raymarch and writes `rgba`; vp_unity_last_status reports how it went).
        GCHandle partsHandle, cubeHandle;
        ulong issuedEvents = 0;        // GL.IssuePluginEvent calls so far; vp_unity_last_status counts the ones that have run
        void IssueFrameOnRenderThread()
        {
            ulong done; int last = vp_unity_last_status(0, out done);
            // completion handshake: the event issued last frame reads `parts` (vp_bin) and writes `rgba` (read-back) whenever the render thread
            // gets to it.  Until the library has counted it (events_run == issued) neither array may be touched and nothing else may run on the
            // context: skip this frame's issue and show the previous texture.
            if (done < issuedEvents) { CompositeParticles(false); return; }      // still present the opaque scene + the previous particles
            if (done > 0) { Check(last, "render-thread frame"); if (last == 0) { filledOnce = true; cubemapResident = true; particlesTex.SetPixelData(rgba, 0); particlesTex.Apply(false); } }
            if (gpuDevices.Length > 1 && rebalanceInterval > 0 && Time.frameCount % rebalanceInterval == 0) vp_rebalance(ctx);   // no event in flight here
            SyncOccluders();                                               // likewise: the context is idle between events
            CompositeParticles();                                          // the image picked up above, over this frame's opaque scene
            bool refill = Time.frameCount % updateInterval == 0 || !filledOnce;
            bool moved = dirLight.transform.rotation != lightOrientation || wsGridCenter != gridCenter.transform.position || !filledOnce;
            if (moved) { lightOrientation = dirLight.transform.rotation; wsGridCenter = gridCenter.transform.position; }
            vp_camera cam; vp_raymarch_params rp;
            CameraAndParams(out cam, out rp);
            int n = refill ? particleSys.GetParticles(parts) : 0;
            if (!partsHandle.IsAllocated) partsHandle = GCHandle.Alloc(parts, GCHandleType.Pinned);    // stays pinned: the event reads it later
            if (!cubeHandle.IsAllocated) cubeHandle = GCHandle.Alloc(cubemapR, GCHandleType.Pinned);
            var fill = FillParams();
            if (!cubemapResident) fill.cubemap = cubeHandle.AddrOfPinnedObject();
            Vector3 g = wsGridCenter;
            var frame = new vp_unity_frame {
                ctx = ctx, flags = (moved ? 1 : 0) | (refill ? 2 : 0), particle_count = n,
                light_to_world = ToArray(dirLight.transform.localToWorldMatrix), grid_center = new float[] { g.x, g.y, g.z },
                psys_local_to_world = ToArray(particleSys.transform.localToWorldMatrix), particles = partsHandle.AddrOfPinnedObject(),
                layout = ParticleLayout(), fill = fill, camera = cam, raymarch = rp };
            if (Check(vp_unity_set_frame_desc(0, ref frame), "vp_unity_set_frame_desc")) { GL.IssuePluginEvent(vp_unity_render_event_func(), 0); issuedEvents++; }
        }

        void UpdateMetavoxelPositions()                                    // VPR.cs:370-394
        {
            Vector3 g = wsGridCenter;
            Check(vp_set_frame(ctx, ToArray(dirLight.transform.localToWorldMatrix), new float[] { g.x, g.y, g.z }), "vp_set_frame");
        }

        // ---- where the particles are (never called from OnPreRender / OnPostRender: the host decides when to refit) ----
        // Moves gridCenter to where the particles uploaded last are: their sphere box in the light's space -> vp_fit_grid -> the GameObject the
        // frame reads.  snap < 0: one voxel (the voxel lattice does not swim when a moving cloud is refitted); 0: no snap.  Returns false when a
        // call failed or the cloud is larger than the grid.
        public bool FitGridToParticles(float snap)
        {
            if (snap < 0f) snap = mvScale.x / (numVoxelsInMetavoxel - 2 * numBorderVoxels);
            vp_particle_bounds b; vp_grid_fit fit;
            if (!Check(vp_particle_bounds(ctx, ToArray(dirLight.transform.worldToLocalMatrix), out b), "vp_particle_bounds") || b.counted == 0) return false;
            int[] n = new int[] { numMetavoxelsX, numMetavoxelsY, numMetavoxelsZ };
            if (!Check(vp_fit_grid(ToArray(dirLight.transform.localToWorldMatrix), b.sphere_min, b.sphere_max, n, mvScale.x, snap, out fit), "vp_fit_grid")) return false;
            gridCenter.transform.position = new Vector3(fit.grid_center[0], fit.grid_center[1], fit.grid_center[2]);   // picked up by the next frame (VPR.cs:189)
            return fit.fits != 0;
        }

        // The reference's AABBForParticles.FindAABB (AABBForParticles.cs:26-62) over the particles uploaded last: the spheres' box in the main
        // camera's space.  Camera space looks down -z: `max` takes the smallest z, `min` the largest (:43-55), as the reference does.
        public Bounds ParticleAABB()
        {
            vp_particle_bounds b;
            if (!Check(vp_particle_bounds(ctx, ToArray(Camera.main.worldToCameraMatrix), out b), "vp_particle_bounds") || b.counted == 0) return new Bounds();
            Vector3 max = new Vector3(b.sphere_max[0], b.sphere_max[1], b.sphere_min[2]);
            Vector3 min = new Vector3(b.sphere_min[0], b.sphere_min[1], b.sphere_max[2]);
            return new Bounds((max + min) / 2.0f, max - min);
        }

        void BinParticlesToMetavoxels()                                    // VPR.cs:397-457
        {
            int n = particleSys.GetParticles(parts);
            var lay = ParticleLayout();
            GCHandle h = GCHandle.Alloc(parts, GCHandleType.Pinned);       // zero-copy view; the library keeps no pointer
            try { Check(vp_bin(ctx, h.AddrOfPinnedObject(), n, ref lay, ToArray(particleSys.transform.localToWorldMatrix)), "vp_bin"); }
            finally { h.Free(); }
        }

        vp_particle_layout ParticleLayout()
        {
            // explicit field offsets: the managed layout of ParticleSystem.Particle is Unity-version specific
            return new vp_particle_layout {
                stride = Marshal.SizeOf(typeof(ParticleSystem.Particle)),
                off_position = (int)Marshal.OffsetOf(typeof(ParticleSystem.Particle), "m_Position"),
                off_size = (int)Marshal.OffsetOf(typeof(ParticleSystem.Particle), "m_Size"),
                off_rotation = (int)Marshal.OffsetOf(typeof(ParticleSystem.Particle), "m_Rotation"),
                off_lifetime = (int)Marshal.OffsetOf(typeof(ParticleSystem.Particle), "m_Lifetime"),
                off_start_lifetime = (int)Marshal.OffsetOf(typeof(ParticleSystem.Particle), "m_StartLifetime"),
                rotation_in_radians = 1 /* the raw field is radians; the .rotation property converts to degrees */ };
        }

        vp_fill_params FillParams()                                        // SetFillPassConstants VPR.cs:523-554
        {
            return new vp_fill_params {
                opacity_factor = opacityFactor, displacement_scale = fDisplacementScale, fade_out_particles = fadeOutParticles ? 1 : 0,
                ambient_r = ambientColor.x, ambient_g = ambientColor.y, ambient_b = ambientColor.z, init_light_intensity = 1.0f,
                light_near = 0.3f, light_far = 1000f, light_cam_distance = 200f, cubemap_size = displacementTexture.width,
                cubemap_format = 1 /* VP_CUBEMAP_R8 */,
                cubemap = IntPtr.Zero, light_depth_map = LightDepthMapPtr() };
        }

        void FillMetavoxels()                                              // VPR.cs:495-520
        {
            var p = FillParams();
            GCHandle h = default(GCHandle);
            if (!cubemapResident) { h = GCHandle.Alloc(cubemapR, GCHandleType.Pinned); p.cubemap = h.AddrOfPinnedObject(); }
            try
            {
                // the cube map only counts as resident after a fill that SUCCEEDED: a failed first fill must upload it again
                if (Check(vp_fill(ctx, ref p), "vp_fill")) { cubemapResident = true; filledOnce = true; }
            }
            finally { if (h.IsAllocated) h.Free(); }
        }

        // The reference's per-metavoxel entry point (VPR.cs:559-609), for a host that drives the fill itself: FillMetavoxelsBegin()
        // (= the head of FillMetavoxels: constants + clear of lightPropogationTex, VPR.cs:497-503), then FillMetavoxel for every
        // occupied metavoxel in zz-major order.
        public void FillMetavoxelsBegin()
        {
            var p = FillParams();
            GCHandle h = default(GCHandle);
            if (!cubemapResident) { h = GCHandle.Alloc(cubemapR, GCHandleType.Pinned); p.cubemap = h.AddrOfPinnedObject(); }
            try { if (Check(vp_fill_begin(ctx, ref p), "vp_fill_begin")) cubemapResident = true; }
            finally { if (h.IsAllocated) h.Free(); }
        }

        public void FillMetavoxel(int xx, int yy, int zz)                  // VPR.cs:559-609
        {
            if (Check(vp_fill_metavoxel(ctx, xx, yy, zz), "vp_fill_metavoxel")) filledOnce = true;
        }

        void CameraAndParams(out vp_camera cam, out vp_raymarch_params rp)  // SetRaymarchPassConstants VPR.cs:716-763
        {
            Camera c = Camera.main;
            Vector3 cp = c.transform.position;
            cam = new vp_camera {
                world_to_camera = ToArray(c.worldToCameraMatrix), camera_to_world = ToArray(c.cameraToWorldMatrix),
                px = cp.x, py = cp.y, pz = cp.z, fov_y = Mathf.Deg2Rad * c.fieldOfView, near_clip = c.nearClipPlane, far_clip = c.farClipPlane };
            rp = new vp_raymarch_params { steps_per_mv = rayMarchSteps, soft_distance = softParticleStepDistance,
                                          scene_depth = SceneDepthPtr(), flags = bShowMetavoxelDrawOrder ? 8 : 0, reserved = new int[3] };
        }

        public void RenderMetavoxels()                                     // VPR.cs:637-713
        {
            if (!filledOnce) return;                                       // nothing filled yet: nothing to march
            vp_camera cam; vp_raymarch_params rp;
            CameraAndParams(out cam, out rp);
            if (!asyncReadback)
            {
                Check(vp_raymarch(ctx, ref cam, ref rp, rgbaHandle.AddrOfPinnedObject()), "vp_raymarch");
                particlesTex.SetPixelData(rgba, 0);
                particlesTex.Apply(false);
                return;
            }
            // last frame's image has had a whole frame to land in `rgba`: show it, then queue this frame's march + copy
            if (imageInFlight && Check(vp_wait_image(ctx), "vp_wait_image")) { particlesTex.SetPixelData(rgba, 0); particlesTex.Apply(false); }
            imageInFlight = Check(vp_raymarch_async(ctx, ref cam, ref rp, rgbaHandle.AddrOfPinnedObject()), "vp_raymarch_async");
        }
        bool imageInFlight = false;

        // The reference's per-metavoxel entry point (VPR.cs:766-794): one metavoxel marched and blended into the library's
        // particlesRT with the blend state of its phase (blendOver: VPR.cs:659-662, else :688-691).  ClearParticlesRT() first
        // (OnPreRender, VPR.cs:171), ReadParticlesRT() after the last one.
        public void ClearParticlesRT() { Check(vp_clear_particles_rt(ctx), "vp_clear_particles_rt"); }
        public void RenderMetavoxel(int xx, int yy, int zz, int orderIndex, bool blendOver)
        {
            vp_camera cam; vp_raymarch_params rp;
            CameraAndParams(out cam, out rp);
            Check(vp_render_metavoxel(ctx, ref cam, ref rp, xx, yy, zz, blendOver ? 1 : 0, orderIndex), "vp_render_metavoxel");
        }
        public void ReadParticlesRT()
        {
            Check(vp_read_particles_rt(ctx, rgbaHandle.AddrOfPinnedObject()), "vp_read_particles_rt");
            particlesTex.SetPixelData(rgba, 0);
            particlesTex.Apply(false);
        }

        // GUI setters (VPR.cs:1040-1119) keep their names
        public void SetOpacityFactor(float v) { opacityFactor = v; }
        public void SetDisplacementScale(float v) { fDisplacementScale = v; }
        public void SetRayMarchSteps(float v) { rayMarchSteps = (int)v; }
        public void SetSoftParticleStepDistance(float v) { softParticleStepDistance = (int)v; }
        public void SetUpdateInterval(float v) { updateInterval = Mathf.Max(1, (int)v); }
        public void SetFadeOutParticles(bool v) { fadeOutParticles = v; }
        public void SetShowMetavoxelDrawOrder(bool show) { bShowMetavoxelDrawOrder = show; }   // VPR.cs:1096-1099
        public void SetCastVolumeShadows(bool v) { castVolumeShadows = v; }                   // added by this binding
        public void SetShadowStrength(float v) { shadowStrength = Mathf.Clamp01(v); }
    }
}
