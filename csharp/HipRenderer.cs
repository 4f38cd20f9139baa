// HipRenderer.cs — drop-in for PTSharpCore.Renderer that runs the per-pixel hot
// path on an MI355X through libptsharp_hip.so (include/ptsharp_hip.h).
//
// Add this file to PTSharpCore/ (same namespace).  It mirrors the reference's
// Renderer factory and knobs (Renderer.cs:35-56), its IterativeRender contract
// (Renderer.cs:702-765) and writes into the same static Buffer (Renderer.PBuffer,
// Buffer.cs:60-97).  P/Invoke follows the conventions the reference already uses
// for its only native dependency, OIDN (OIDN.cs:43-95): Cdecl, IntPtr handles,
// create / commit / execute / release, error strings fetched after a failure.
//
// NOTE: this file is not compiled in this repository (no .NET SDK in the build
// image); the same ABI is exercised from Python/ctypes by tests/test_abi.py and
// the GPU parity suite.  Struct layouts below match ptsharp_hip.h field by field.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using System.Threading.Tasks;
using SkiaSharp;

namespace PTSharpCore
{
    internal static class PtHip
    {
        const string Lib = "ptsharp_hip";   // libptsharp_hip.so on Linux

        public const int PT_OK = 0;
        public const int PT_ERR_UNSUPPORTED = -4;
        public const int PT_PASS_KERNEL_TIMING = 1, PT_PASS_SERIAL = 2;
        public const int PT_MARCH_LANE = 1, PT_MARCH_WAVE = 2;   // pt_intersect / pt_occluded flags
        public const int PT_IMAGE_RGB8 = 0, PT_IMAGE_RGBA8 = 1;  // pt_image_format (pt_read_image)
        public const int PT_FEATURE_ALBEDO_F64 = 0, PT_FEATURE_NORMAL_F32 = 1, PT_FEATURE_DEPTH_F64 = 2, PT_FEATURE_KIND_I32 = 3, PT_FEATURE_MATERIAL_I32 = 4;  // pt_feature
        public const int PT_DENOISED_RGB8 = 0, PT_DENOISED_RGBA8 = 1, PT_DENOISED_COLOUR_F64 = 2, PT_DENOISED_VARIANCE_F64 = 3;  // pt_denoised_format
        public const int SHAPE_SPHERE = 0, SHAPE_CUBE = 1, SHAPE_PLANE = 2, SHAPE_TRIANGLE = 3, SHAPE_MESH = 4;
        public const int SHAPE_SDF = 5, SHAPE_VOLUME = 6, SHAPE_TRANSFORMED = 7;

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_texture
        {
            public int width; public int height; public IntPtr data;   // ColorTexture.Data as [h][w][3] double
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_material
        {
            public fixed double color[3];
            public double emittance, index, gloss, tint, reflectivity;
            public int transparent;
            public int texture, normal_texture, bump_texture, gloss_texture;   // 1-based into textures, 0 = null
            public int _pad;
            public double bump_multiplier;
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_sdf_node
        {
            public int op, num_children, first_child, _pad;
            public fixed double @params[8];
            public fixed double matrix[16];
            public fixed double inverse[16];
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_sdf_shape { public int root, material; }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_volume_window { public double lo, hi; public int material, _pad; }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_volume
        {
            public int w, h, d;
            public int num_windows;
            public double zscale;
            public IntPtr data;
            public IntPtr windows;
            public fixed float box_min[3];
            public fixed float box_max[3];
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_transformed_shape
        {
            public int shape_kind, shape_index;
            public fixed double matrix[16];
            public fixed double inverse[16];
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_scene_desc
        {
            public int num_materials; public IntPtr materials;
            public int num_shapes; public IntPtr shape_kind; public IntPtr shape_index;
            public int num_spheres; public IntPtr sphere_center; public IntPtr sphere_radius; public IntPtr sphere_material;
            public int num_cubes; public IntPtr cube_min; public IntPtr cube_max; public IntPtr cube_material;
            public int num_planes; public IntPtr plane_point; public IntPtr plane_normal; public IntPtr plane_material;
            public int num_triangles; public IntPtr tri_v1, tri_v2, tri_v3, tri_n1, tri_n2, tri_n3; public IntPtr tri_material;
            public int num_meshes; public IntPtr mesh_first; public IntPtr mesh_count;
            public fixed double env_color[3];
            public int num_textures; public IntPtr textures;
            public IntPtr tri_t1, tri_t2, tri_t3;
            public int env_texture; public int _pad; public double env_texture_angle;
            public int num_sdf_nodes; public IntPtr sdf_nodes; public IntPtr sdf_children;
            public int num_sdf_shapes; public IntPtr sdf_shapes;
            public int num_volumes; public IntPtr volumes;
            public int num_transformed; public IntPtr transformed;
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_camera
        {
            public fixed float p[3]; public fixed float u[3]; public fixed float v[3]; public fixed float w[3];
            public double m, focal_distance, aperture_radius;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_sampler
        {
            public int first_hit_samples, max_bounces, direct_lighting, soft_shadows, light_mode, specular_mode;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_pass_params
        {
            public int spp, stratified;
            public ulong seed;
            public uint pass_index;
            public int num_tiles;
            public IntPtr tiles;
            public int engine, flags;
            public int adaptive_samples, firefly_samples;   // Renderer.AdaptiveSamples / FireflySamples
            public int passes;                              // K consecutive passes in one call (0/1: one)
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_device_opts { public int device, width, height; }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_stats
        {
            public ulong rays, rays_total; public double last_pass_ms, total_ms;
            public ulong bvh_nodes, bvh_bytes; public double build_ms; public ulong passes;
            public ulong shadow_rays;
            public fixed double kernel_ms[8];       // PT_K_SLOTS
            public fixed uint kernel_launches[8];
            public ulong traversal_bytes;           // BVH nodes + leaf chunks (what traversal reads)
            public ulong tail_handoffs;             // shadow refill kernel's tail hand-offs, last pass (ABI 9)
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_trace_counters
        {
            public ulong rays, nodes_visited, prims_tested, shading_fetches, shadow_rays, shadow_nodes, shadow_prims;
            public ulong lit_shadow_rays, accum_runs;
            public ulong volume_samples, sdf_evals;   // Volume.Intersect / SDFShape.Intersect march steps
            public fixed ulong march_clock[8];   // the Volume march's phase clocks (counted passes)
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_denoise_params
        {
            public int iterations;       // 1..8
            public int reserved;         // 0
            public double sigma_colour;  // > 0, finite
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_denoise_guided_params
        {
            public int iterations;       // 1..8
            public int reserved;         // 0
            public double sigma_colour;  // > 0, finite
            public double sigma_normal;  // >= 0, finite; 0 = term off
            public double sigma_albedo;  // likewise
            public double sigma_depth;   // likewise; relative to the centre's depth
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_temporal_params
        {
            public int max_history;      // 0..2^20
            public int reserved;         // 0
            public double sigma_depth;   // >= 0, finite; 0 = depth test off
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_mesh_data
        {
            public int num_triangles;
            public IntPtr v1, v2, v3, n1, n2, n3, t1, t2, t3;   // [n][3] float, owned by the library
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_shape_update
        {
            public int num_spheres, num_cubes, num_transformed, reserved;   // reserved = 0
            public IntPtr sphere_center;   // [num_spheres][3] float; null = spheres stay
            public IntPtr sphere_radius;   // [num_spheres] double;   null = radii stay
            public IntPtr cube_min;        // [num_cubes][3] float;   both or neither
            public IntPtr cube_max;
            public IntPtr xform_matrix;    // [num_transformed][16] double, row-major; both or neither
            public IntPtr xform_inverse;
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_mesh_update
        {
            public int num_triangles;      // must equal the uploaded scene's
            public int normals_mode;       // 0: n1..n3 given or kept (all null); PT_NORMALS_FACE; PT_NORMALS_SMOOTH
            public fixed int reserved[2];  // 0
            public IntPtr v1, v2, v3;      // [n][3] float, required
            public IntPtr n1, n2, n3;      // [n][3] float; only with normals_mode 0
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_hit_arrays
        {
            // every pointer may be IntPtr.Zero: that output is not wanted
            public fixed int reserved[2];  // 0
            public IntPtr t;               // [n] double: Hit.T, 1e9 on a miss
            public IntPtr kind;            // [n] int: the pt_shape_kind hit, or -1
            public IntPtr index;           // [n] int: index into that kind's arrays; the source triangle for a triangle
            public IntPtr prim;            // [n] int: the source triangle whose surface was hit, or -1
            public IntPtr shape;           // [n] int: the slot in Scene.Shapes order
            public IntPtr position;        // [n][3] float: Hit.Info's Position
            public IntPtr normal;          // [n][3] float: Hit.Info's Normal after the flip
            public IntPtr inside;          // [n] int: Hit.Info's Inside
            public IntPtr material;        // [n] int: the material id
            public IntPtr albedo;          // [n][3] double: the MaterialAt colour; on a miss the environment
            public IntPtr gloss;           // [n] double: the MaterialAt gloss
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_mesh_pose
        {
            public int num_meshes;         // must equal the uploaded scene's num_meshes
            public int normals_mode;       // 0: Mesh.Transform's (MulDirection of the rest normals); PT_NORMALS_FACE; PT_NORMALS_SMOOTH
            public fixed int reserved[2];  // 0
            public IntPtr matrices;        // [num_meshes][16] double, row-major, required
            public IntPtr mesh_mask;       // [num_meshes] int or null (= all); 0: the mesh takes its rest values verbatim
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_skin_desc
        {
            public int num_triangles;      // must equal the uploaded scene's num_triangles
            public int num_bones;          // 1..PT_SKIN_MAX_BONES
            public fixed int reserved[2];  // 0
            public IntPtr bone1, bone2, bone3;        // [num_triangles][4] int each: the bones of corner 1, 2, 3, every one in [0, num_bones)
            public IntPtr weight1, weight2, weight3;  // [num_triangles][4] float each: their weights; +-0: the influence is dead
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_mesh_skin
        {
            public int num_bones;          // must equal the installed skin's num_bones
            public int normals_mode;       // 0: the blend of MulDirection of the rest normals; PT_NORMALS_FACE; PT_NORMALS_SMOOTH
            public fixed int reserved[2];  // 0
            public IntPtr matrices;        // [num_bones][16] double, row-major, required
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_morph_desc
        {
            public int num_triangles;      // must equal the uploaded scene's num_triangles
            public int num_targets;        // 1..PT_MORPH_MAX_TARGETS
            public fixed int reserved[2];  // 0
            public IntPtr target_first;    // [num_targets + 1] long, target_first[0] = 0, non-decreasing; the last = number of deltas
            public IntPtr corner;          // [deltas] int: 3 * triangle + c, strictly ascending within a target
            public IntPtr dpos;            // [deltas][3] float
            public IntPtr dnrm;            // [deltas][3] float or null: the morph carries no normal deltas
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_mesh_morph
        {
            public int num_targets;        // must equal the installed morph's
            public int normals_mode;       // 0, PT_NORMALS_FACE, PT_NORMALS_SMOOTH
            public int num_bones;          // 0 when skin_matrices is null, else the installed skin's
            public int reserved;           // 0
            public IntPtr weights;         // [num_targets] float, required
            public IntPtr skin_matrices;   // null: morph only; else [num_bones][16] double: morph, then the skin of the morphed pose
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_volume_update
        {
            public int num_volumes;        // must equal the uploaded scene's
            public fixed int reserved[3];  // 0
            public IntPtr data;            // null, or [num_volumes] pointers: null = the volume keeps its voxels, else [d][h][w] double
            public IntPtr windows;         // null, or [num_volumes] pointers: null = kept, else the uploaded num_windows pt_volume_window
        }

        public const int PT_LOOK_ENV = 1;   // pt_material_update.flags
        public const int PT_TEXELS_F64 = 0, PT_TEXELS_RGB8 = 1, PT_TEXELS_RGBA8 = 2;   // pt_texel_format

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_material_update
        {
            public int num_materials;      // must equal the uploaded scene's
            public int flags;              // 0 or PT_LOOK_ENV: the env_* fields are taken
            public fixed int reserved[2];  // 0
            public IntPtr materials;       // [num_materials] pt_material, or null = kept
            public fixed double env_color[3];
            public int env_texture, _pad;  // 1-based, 0 = null
            public double env_texture_angle;
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_look_info
        {
            public int num_materials, num_textures, num_lights;
            public int lights_lean, route, shade_route;
            public int env_texture, _pad;
            public fixed double env_color[3];
            public double env_texture_angle;
        }

        [StructLayout(LayoutKind.Sequential)]
        public struct pt_texture_image
        {
            public int width, height;      // must equal the uploaded texture's
            public int format, reserved;   // pt_texel_format; 0
            public IntPtr data;            // F64: [h][w][3] double; RGB8 / RGBA8: [h][w][3|4] bytes, rows packed
            public IntPtr lut;             // [256] double, required for the 8-bit formats
        }

        [StructLayout(LayoutKind.Sequential)]
        public unsafe struct pt_texture_update
        {
            public int num_textures;       // must equal the uploaded scene's
            public fixed int reserved[3];  // 0
            public IntPtr images;          // null, or [num_textures] pointers to pt_texture_image: null = the texture stays
        }

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_get_version();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_device_count(out int count);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_create(ref pt_device_opts opts, out IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_upload_scene(IntPtr ctx, ref pt_scene_desc scene);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_render_pass(IntPtr ctx, ref pt_camera cam, ref pt_sampler smp, ref pt_pass_params pass);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_render_pass_counted(IntPtr ctx, ref pt_camera cam, ref pt_sampler smp, ref pt_pass_params pass, out pt_trace_counters counters);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_synchronize(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_buffer(IntPtr ctx, double[] m, double[] v, int[] n);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_write_buffer(IntPtr ctx, double[] m, double[] v, int[] n);
        // channel: (int)Channel (Buffer.cs:8-16 = pt_channel); format: PT_IMAGE_RGB8 / PT_IMAGE_RGBA8 (ABI 10)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_image(IntPtr ctx, int channel, int format, byte[] rgb);
        // the variance-guided à-trous denoiser (Renderer.Denoise; not OIDN): filter the Buffer as it stands, read the result
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_denoise(IntPtr ctx, ref pt_denoise_params p, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_denoised(IntPtr ctx, int format, IntPtr dst);
        // first-hit features (albedo, shading normal, depth, kind, material: one primary ray per pixel) and the filter guided by them
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_render_features(IntPtr ctx, ref pt_camera cam, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_features(IntPtr ctx, int feature, IntPtr dst);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_write_features(IntPtr ctx, double[] albedo, float[] normal, double[] depth, int[] kind);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_denoise_guided(IntPtr ctx, ref pt_denoise_guided_params p, out double kernelMs);
        // motion vectors and temporal accumulation across animated frames (pt_motion_array: PT_MOTION_*)
        public const int PT_MOTION_SHAPE_I32 = 0, PT_MOTION_PRIM_I32 = 1, PT_MOTION_DEPTH_F64 = 2, PT_MOTION_PREV_XY_F64 = 3,
                         PT_MOTION_PREV_DEPTH_F64 = 4, PT_MOTION_PREV_PIXEL_I32 = 5, PT_MOTION_STATUS_I32 = 6;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_motion_snapshot(IntPtr ctx, ref pt_camera cam);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_render_motion(IntPtr ctx, ref pt_camera cam, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_motion(IntPtr ctx, int what, IntPtr dst);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_accumulate_temporal(IntPtr ctx, ref pt_temporal_params p, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_temporal(IntPtr ctx, double[] m, double[] v, int[] n, int[] status);
        // plain: a pt_denoise_params*, or guided: a pt_denoise_guided_params*; the other IntPtr.Zero
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_denoise_temporal(IntPtr ctx, IntPtr plain, IntPtr guided, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_reset_temporal(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_tiles(IntPtr ctx, int[] tiles, int num_tiles, double[] m, double[] v, int[] n);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_write_tiles(IntPtr ctx, int[] tiles, int num_tiles, double[] m, double[] v, int[] n);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_reset_buffer(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_stats_get(IntPtr ctx, out pt_stats stats);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_scene_bvh_digest(ref pt_scene_desc scene, ulong[] out4);
        // Scene.Intersect of a batch of rays / the shadow query against a t (PT_MARCH_* flags: the Volume march form)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_triangles(IntPtr ctx, int numTriangles, float[] v1, float[] v2, float[] v3, float[] n1, float[] n2, float[] n3, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_tri_bvh(IntPtr ctx, long[] counts, uint[] nodes, uint[] chunks, uint[] records, float[] box);
        public const int PT_NORMALS_FACE = 1, PT_NORMALS_SMOOTH = 2;   // pt_normals_mode
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_triangles_normals(IntPtr ctx, int numTriangles, float[] v1, float[] v2, float[] v3, int mode, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_tri_normals(IntPtr ctx, float[] n1, float[] n2, float[] n3);
        // new sphere, cube and TransformedShape parameters: the analytic BVH refitted on the device
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_shapes(IntPtr ctx, ref pt_shape_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_shape_bvh(IntPtr ctx, long[] counts, uint[] nodes, uint[] recs, uint[] heavy, double[] lights);
        // pt_update_triangles / _normals for a scene with instanced meshes too: their BLASes refitted on the device
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_meshes(IntPtr ctx, ref pt_mesh_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_blas(IntPtr ctx, long[] counts, int[] blas, uint[] nodes, uint[] recs, uint[] shade, float[] innerBoxes);
        // Mesh.Transform on the device: a rest pose kept there, one matrix per mesh per call, then pt_update_meshes' refits
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_set_rest_pose(IntPtr ctx, int numTriangles, float[] v1, float[] v2, float[] v3, float[] n1, float[] n2, float[] n3);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_pose_meshes(IntPtr ctx, ref pt_mesh_pose u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_pose(IntPtr ctx, float[] v1, float[] v2, float[] v3, float[] n1, float[] n2, float[] n3);
        // Blend skinning on the device: four bones and weights per corner sent once, one matrix per bone per call, then pt_update_meshes' refits
        public const int PT_SKIN_INFLUENCES = 4, PT_SKIN_MAX_BONES = 65536;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_set_skin(IntPtr ctx, ref pt_skin_desc desc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_skin_meshes(IntPtr ctx, ref pt_mesh_skin u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_skin(IntPtr ctx, int[] bone1, int[] bone2, int[] bone3, float[] weight1, float[] weight2, float[] weight3);
        // Morph targets on the device: sparse per-corner deltas sent once, one weight per target per call (and optionally the skin's matrices), then pt_update_meshes' refits
        public const int PT_MORPH_MAX_TARGETS = 65535;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_set_morph(IntPtr ctx, ref pt_morph_desc desc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_morph_meshes(IntPtr ctx, ref pt_mesh_morph u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_morph(IntPtr ctx, long[] counts3, long[] targetFirst, int[] corner, float[] dpos, float[] dnrm);
        // pt_update_meshes that also re-sorts the world triangle BVH on the device (u = IntPtr.Zero: the staged pose, skin or morph), and the tree's cost
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_rebuild_meshes(IntPtr ctx, ref pt_mesh_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_rebuild_meshes(IntPtr ctx, IntPtr u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_tri_bvh_cost(IntPtr ctx, double[] out3);
        public const int PT_REBUILD_WORLD = 1, PT_REBUILD_BLAS = 2;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_rebuild_blas(IntPtr ctx, ref pt_mesh_update u, int what, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_rebuild_blas(IntPtr ctx, IntPtr u, int what, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_blas_cost(IntPtr ctx, int numBlas, double[] out3PerBlas);
        // new voxels and iso-windows for the scene's Volumes: their derived tables rebuilt on the device (DESIGN.md §4i)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_volumes(IntPtr ctx, ref pt_volume_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_materials(IntPtr ctx, ref pt_material_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_materials(IntPtr ctx, out pt_look_info info, [In, Out] pt_material[] materials, int[] lightRows, double[] lightSpheres);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_update_textures(IntPtr ctx, ref pt_texture_update u, out double kernelMs);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_texture(IntPtr ctx, int index, int[] info, double[] data);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_read_volume(IntPtr ctx, int index, long[] info, double[] data, [In, Out] pt_volume_window[] windows, sbyte[] runs, double[] cells);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_intersect(IntPtr ctx, long n, float[] origins, float[] dirs, int flags, double[] t, int[] kind);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_occluded(IntPtr ctx, long n, float[] origins, float[] dirs, double[] tMax, int flags, int[] blocked);
        // what a host's rays hit and where: identity in the host's numbering and Hit.Info (DESIGN.md §4h)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_intersect_hits(IntPtr ctx, long n, float[] origins, float[] dirs, int flags, ref pt_hit_arrays arrays);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_query_kernel_ms(IntPtr ctx, out double ms);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr pt_last_error();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void pt_destroy(IntPtr ctx);
        // multi-GPU (include/ptsharp_hip.h "Multi-GPU"): one process per GPU (unique id + init per rank) or
        // one process driving G contexts (init_all / gather_all)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_unique_id(byte[] id128);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_init(IntPtr ctx, int nranks, int rank, byte[] id128);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_gather(IntPtr ctx, int root);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_destroy(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_init_all(IntPtr[] ctxs, int n);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_comm_gather_all(IntPtr[] ctxs, int n, int root);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_gather_layout(int nranks, int root, int[] counts, int imageTiles, long[] offsets, out long total);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_tile_lists_check(int[] ids, long n, int imageTiles);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl, CharSet = CharSet.Ansi)] public static extern int pt_obj_load(string path, out pt_mesh_data mesh);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void pt_mesh_free(ref pt_mesh_data mesh);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern IntPtr pt_obj_last_error();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int pt_mesh_smooth_normals(int n, float[] v1, float[] v2, float[] v3, float[] n1, float[] n2, float[] n3);

        public static void Check(int rc, string where)
        {
            if (rc != PT_OK)
                throw new InvalidOperationException($"{where} failed ({rc}): {Marshal.PtrToStringAnsi(pt_last_error())}");
        }
    }

    /// <summary>Renderer drop-in: same factory, knobs and IterativeRender contract as Renderer.</summary>
    class HipRenderer : IDisposable
    {
        Scene Scene; Camera Camera; DefaultSampler Sampler;
        public int SamplesPerPixel = 2;           // Renderer.cs:42
        public bool StratifiedSampling = false;   // Renderer.cs:44
        public int AdaptiveSamples = 0;           // Renderer.cs:23, phase at :340-410
        public int FireflySamples = 0;            // Renderer.cs:26, phase at :412-470
        public ulong Seed = 0;                     // Random.Shared is unseedable; this keys the GPU stream
        public int NumCPU = Environment.ProcessorCount;   // Renderer.cs:51-54: 1 selects Render() in IterativeRender
        /// <summary>32x32 tiles this renderer draws (tile id = ty * ceil(W/32) + tx); null = the whole
        /// image.  A multi-GPU rank draws TilesForRank(W, H, rank, world) (SURVEY.md §8e).</summary>
        public int[] Tiles = null;
        /// <summary>IterativeRender takes each pass' image from ReadImage (pt_read_image: the channel resolved
        /// on the device, 4 B per pixel copied back instead of 52) and fills Renderer.PBuffer once, after
        /// the last pass.  False keeps the ReadBuffer + Buffer.Image path after every pass.</summary>
        public bool DeviceImages = false;
        /// <summary>Renderer.Denoise (Renderer.cs:731-761): IterativeRender also writes albedo_channel.png,
        /// normal_channel.png and denoised_output.png after each pass, into pathTemplate's directory, and
        /// returns the denoised image.  The denoiser is the library's variance-guided à-trous filter
        /// (pt_denoise), not OIDN.</summary>
        public bool Denoise = false;
        public int DenoiseIterations = 5;         // 1..8
        public double DenoiseSigmaColour = 4.0;
        /// <summary>With Denoise: the first-hit features are rendered once (RenderFeatures) and the filter is
        /// pt_denoise_guided, whose tap weights also fall with the albedo, normal and depth distance to the
        /// centre.</summary>
        public bool DenoiseGuided { get; set; } = false;
        public double DenoiseSigmaNormal = 0.3, DenoiseSigmaAlbedo = 0.3, DenoiseSigmaDepth = 0.1;   // 0 = term off
        bool haveFeatures = false;
        internal IntPtr ctx;
        int W, H, pass;
        internal int Width => W;
        internal int Height => H;
        bool uploaded;
        readonly List<GCHandle> pins = new();

        // DefaultSampler keeps FirstHitSamples/MaxBounces/DirectLighting/SoftShadows private
        // (Sampler.cs:13-16): the caller passes the values it constructed the sampler with.
        int firstHit, maxBounces; bool directLighting = true, softShadows = true;

        public static HipRenderer NewRenderer(Scene scene, Camera camera, DefaultSampler sampler, int firstHitSamples,
                                              int maxBounces, int w, int h, int device = 0, bool multithreaded = true)
        {
            var r = new HipRenderer { Scene = scene, Camera = camera, Sampler = sampler, W = w, H = h,
                                      firstHit = firstHitSamples, maxBounces = maxBounces,
                                      NumCPU = multithreaded ? Environment.ProcessorCount : 1 };
            Renderer.PBuffer = new Buffer(w, h);
            var opts = new PtHip.pt_device_opts { device = device, width = w, height = h };
            PtHip.Check(PtHip.pt_create(ref opts, out r.ctx), "pt_create");
            return r;
        }

        IntPtr Pin(Array a) { var g = GCHandle.Alloc(a, GCHandleType.Pinned); pins.Add(g); return g.AddrOfPinnedObject(); }

        /// <summary>Static interleaved tile ownership: tile t belongs to rank t % world.  Every pixel's
        /// random stream is keyed by the pixel, so the union of the ranks' Buffers is the 1-GPU Buffer, bit
        /// for bit (pt_comm_gather sums the disjoint tiles).</summary>
        public static int[] TilesForRank(int w, int h, int rank, int world)
        {
            int n = ((w + 31) / 32) * ((h + 31) / 32);
            var t = new List<int>();
            for (int i = rank; i < n; i += world) t.Add(i);
            return t.ToArray();
        }

        // Flatten Scene.Shapes (Scene.cs:19) with a type switch; returns PT_ERR_UNSUPPORTED kinds as exceptions
        // so the caller can fall back to the CPU Renderer.
        unsafe void Upload()
        {
            // ColorTexture instances (Texture.cs:96-252) by reference; 1-based ids, 0 = null.
            var texs = new List<PtHip.pt_texture>(); var texIds = new Dictionary<ITexture, int>(ReferenceEqualityComparer.Instance);
            int Tid(ITexture t)
            {
                if (t == null) return 0;
                if (t is not ColorTexture ct) throw new NotSupportedException($"{t.GetType().Name} is not on the GPU path");
                if (!texIds.TryGetValue(t, out int id))
                {
                    var data = new double[3 * ct.Data.Length];
                    for (int i = 0; i < ct.Data.Length; i++) { data[3 * i] = ct.Data[i].r; data[3 * i + 1] = ct.Data[i].g; data[3 * i + 2] = ct.Data[i].b; }
                    texs.Add(new PtHip.pt_texture { width = ct.Width, height = ct.Height, data = Pin(data) });
                    id = texs.Count; texIds[t] = id;
                }
                return id;
            }
            var mats = new List<PtHip.pt_material>(); var matIds = new Dictionary<Material, int>();
            int Mid(Material m)
            {
                if (!matIds.TryGetValue(m, out int id))
                {
                    id = mats.Count; matIds[m] = id;
                    var pm = new PtHip.pt_material { emittance = m.Emittance, index = m.Index, gloss = m.Gloss, tint = m.Tint,
                        reflectivity = m.Reflectivity, transparent = m.Transparent ? 1 : 0,
                        texture = Tid(m.Texture), normal_texture = Tid(m.NormalTexture), bump_texture = Tid(m.BumpTexture),
                        gloss_texture = Tid(m.GlossTexture), bump_multiplier = m.BumpMultiplier };
                    pm.color[0] = m.Color.r; pm.color[1] = m.Color.g; pm.color[2] = m.Color.b;
                    mats.Add(pm);
                }
                return id;
            }
            var kind = new List<int>(); var index = new List<int>();
            var sc = new List<float>(); var sr = new List<double>(); var sm = new List<int>();
            var cmin = new List<float>(); var cmax = new List<float>(); var cm = new List<int>();
            var pp = new List<float>(); var pn = new List<float>(); var pm = new List<int>();
            var v1 = new List<float>(); var v2 = new List<float>(); var v3 = new List<float>();
            var n1 = new List<float>(); var n2 = new List<float>(); var n3 = new List<float>(); var tm = new List<int>();
            var t1 = new List<float>(); var t2 = new List<float>(); var t3 = new List<float>();
            var mf = new List<int>(); var mc = new List<int>();
            void Add3(List<float> l, Vector v) { l.Add((float)v.X); l.Add((float)v.Y); l.Add((float)v.Z); }
            // SDF trees, volumes and transformed shapes (§8f row 4).  SDF / Volume / TransformedShape keep
            // their fields private in the reference (SDF.cs, Volume.cs:21-27, TransformedShape.cs:11-13):
            // the integration marks them `internal` (INTEGRATION.md), as for Plane.
            var sdfNodes = new List<PtHip.pt_sdf_node>(); var sdfKids = new List<int>(); var sdfIds = new Dictionary<SDF, int>(ReferenceEqualityComparer.Instance);
            var meshIds = new Dictionary<IShape, int>(ReferenceEqualityComparer.Instance);
            var sdfShapes = new List<PtHip.pt_sdf_shape>(); var vols = new List<PtHip.pt_volume>(); var xfs = new List<PtHip.pt_transformed_shape>();
            void Mat16(double* dst, Matrix m)
            {
                double[] a = { m.M11, m.M12, m.M13, m.M14, m.M21, m.M22, m.M23, m.M24, m.M31, m.M32, m.M33, m.M34, m.M41, m.M42, m.M43, m.M44 };
                for (int k = 0; k < 16; k++) dst[k] = a[k];
            }
            int Sdf(SDF n)
            {
                if (sdfIds.TryGetValue(n, out int id)) return id;
                var node = new PtHip.pt_sdf_node();
                SDF[] kids = n switch
                {
                    TransformSDF t => new[] { t.SDF }, ScaleSDF sc => new[] { sc.SDF }, RepeatSDF r => new[] { r.SDF },
                    UnionSDF u => u.Items, DifferenceSDF df => df.Items, IntersectionSDF i => i.Items, _ => Array.Empty<SDF>(),
                };
                var kidIds = new List<int>(); foreach (var k in kids) kidIds.Add(Sdf(k));
                node.num_children = kidIds.Count; node.first_child = sdfKids.Count; sdfKids.AddRange(kidIds);
                switch (n)
                {
                    case SphereSDF sp: node.op = 0; node.@params[0] = sp.Radius; node.@params[1] = sp.Exponent; break;
                    case CubeSDF cu: node.op = 1; node.@params[0] = cu.Size.X; node.@params[1] = cu.Size.Y; node.@params[2] = cu.Size.Z; break;
                    case CylinderSDF cy: node.op = 2; node.@params[0] = cy.Radius; node.@params[1] = cy.Height; break;
                    case CapsuleSDF ca: node.op = 3; node.@params[0] = ca.A.X; node.@params[1] = ca.A.Y; node.@params[2] = ca.A.Z;
                        node.@params[3] = ca.B.X; node.@params[4] = ca.B.Y; node.@params[5] = ca.B.Z; node.@params[6] = ca.Radius; node.@params[7] = ca.Exponent; break;
                    case TorusSDF to: node.op = 4; node.@params[0] = to.MajorRadius; node.@params[1] = to.MinRadius;
                        node.@params[2] = to.MajorExponent; node.@params[3] = to.MinorExponent; break;
                    case TransformSDF tr: node.op = 5; Mat16(node.matrix, tr.Matrix); Mat16(node.inverse, tr.Inverse); break;
                    case ScaleSDF sc: node.op = 6; node.@params[0] = sc.Factor; break;
                    case UnionSDF: node.op = 7; break;
                    case DifferenceSDF: node.op = 8; break;
                    case IntersectionSDF: node.op = 9; break;
                    case RepeatSDF re: node.op = 10; node.@params[0] = re.Step.X; node.@params[1] = re.Step.Y; node.@params[2] = re.Step.Z; break;
                    default: throw new NotSupportedException($"{n.GetType().Name} is not on the GPU path");
                }
                id = sdfNodes.Count; sdfIds[n] = id; sdfNodes.Add(node);
                return id;
            }
            (int, int) Inner(IShape s)
            {
                switch (s)
                {
                    case Sphere sp: Add3(sc, sp.Center); sr.Add(sp.Radius); sm.Add(Mid(sp.Material)); return (PtHip.SHAPE_SPHERE, sr.Count - 1);
                    case Cube cu: Add3(cmin, cu.Min); Add3(cmax, cu.Max); cm.Add(Mid(cu.Material)); return (PtHip.SHAPE_CUBE, cm.Count - 1);
                    case Plane pl: Add3(pp, pl.Point); Add3(pn, pl.Normal); pm.Add(Mid(pl.Material)); return (PtHip.SHAPE_PLANE, pm.Count - 1);
                    case SDFShape sd: sdfShapes.Add(new PtHip.pt_sdf_shape { root = Sdf(sd.SDF), material = Mid(sd.Material) }); return (PtHip.SHAPE_SDF, sdfShapes.Count - 1);
                    case Volume vo:
                    {
                        var wins = new PtHip.pt_volume_window[vo.Windows.Length];
                        for (int k = 0; k < wins.Length; k++)
                            wins[k] = new PtHip.pt_volume_window { lo = vo.Windows[k].Lo, hi = vo.Windows[k].Hi, material = Mid(vo.Windows[k].VolumeWindowMaterial) };
                        var v = new PtHip.pt_volume { w = vo.W, h = vo.H, d = vo.D, num_windows = wins.Length, zscale = vo.ZScale,
                                                      data = Pin(vo.Data), windows = Pin(wins) };
                        v.box_min[0] = (float)vo.Box.Min.X; v.box_min[1] = (float)vo.Box.Min.Y; v.box_min[2] = (float)vo.Box.Min.Z;
                        v.box_max[0] = (float)vo.Box.Max.X; v.box_max[1] = (float)vo.Box.Max.Y; v.box_max[2] = (float)vo.Box.Max.Z;
                        vols.Add(v);
                        return (PtHip.SHAPE_VOLUME, vols.Count - 1);
                    }
                    case Mesh me:   // instanced: the mesh's triangles in object space, one BLAS per distinct mesh
                    {
                        if (!meshIds.TryGetValue(s, out int id))
                        {
                            id = mf.Count; mf.Add(tm.Count); mc.Add(me.Triangles.Length);
                            foreach (var t in me.Triangles) AddTri(t);
                            meshIds[s] = id;
                        }
                        return (PtHip.SHAPE_MESH, id);
                    }
                    default: throw new NotSupportedException($"{s.GetType().Name} inside a TransformedShape is not on the GPU path");
                }
            }
            void AddTri(Triangle t)
            {
                Add3(v1, t.V1); Add3(v2, t.V2); Add3(v3, t.V3); Add3(n1, t.N1); Add3(n2, t.N2); Add3(n3, t.N3);
                Add3(t1, t.T1); Add3(t2, t.T2); Add3(t3, t.T3);
                tm.Add(Mid(t.Material));
            }
            foreach (var s in Scene.Shapes)
            {
                switch (s)
                {
                    case Sphere sp: kind.Add(PtHip.SHAPE_SPHERE); index.Add(sr.Count); Add3(sc, sp.Center); sr.Add(sp.Radius); sm.Add(Mid(sp.Material)); break;
                    case Cube cu: kind.Add(PtHip.SHAPE_CUBE); index.Add(cm.Count); Add3(cmin, cu.Min); Add3(cmax, cu.Max); cm.Add(Mid(cu.Material)); break;
                    // Plane.Point/Normal/Material are private in the reference (Plane.cs:9-11): the integration
                    // marks them `internal`, the same visibility Sphere and Cube already use (INTEGRATION.md).
                    case Plane pl: kind.Add(PtHip.SHAPE_PLANE); index.Add(pm.Count); Add3(pp, pl.Point); Add3(pn, pl.Normal); pm.Add(Mid(pl.Material)); break;
                    case Triangle tr: kind.Add(PtHip.SHAPE_TRIANGLE); index.Add(tm.Count); AddTri(tr); break;
                    case SDFShape or Volume: { var (k, i) = Inner(s); kind.Add(k); index.Add(i); break; }
                    case TransformedShape ts:
                    {
                        var (k, i) = Inner(ts.Shape);
                        var x = new PtHip.pt_transformed_shape { shape_kind = k, shape_index = i };
                        Mat16(x.matrix, ts.Matrix); Mat16(x.inverse, ts.Inverse);
                        kind.Add(PtHip.SHAPE_TRANSFORMED); index.Add(xfs.Count); xfs.Add(x);
                        break;
                    }
                    case Mesh me: kind.Add(PtHip.SHAPE_MESH); index.Add(mf.Count); mf.Add(tm.Count); mc.Add(me.Triangles.Length); foreach (var t in me.Triangles) AddTri(t); break;
                    default: throw new NotSupportedException($"{s.GetType().Name} is not on the GPU path");
                }
            }
            var d = new PtHip.pt_scene_desc
            {
                num_materials = mats.Count, materials = Pin(mats.ToArray()),
                num_shapes = kind.Count, shape_kind = Pin(kind.ToArray()), shape_index = Pin(index.ToArray()),
                num_spheres = sr.Count, sphere_center = Pin(sc.ToArray()), sphere_radius = Pin(sr.ToArray()), sphere_material = Pin(sm.ToArray()),
                num_cubes = cm.Count, cube_min = Pin(cmin.ToArray()), cube_max = Pin(cmax.ToArray()), cube_material = Pin(cm.ToArray()),
                num_planes = pm.Count, plane_point = Pin(pp.ToArray()), plane_normal = Pin(pn.ToArray()), plane_material = Pin(pm.ToArray()),
                num_triangles = tm.Count, tri_v1 = Pin(v1.ToArray()), tri_v2 = Pin(v2.ToArray()), tri_v3 = Pin(v3.ToArray()),
                tri_n1 = Pin(n1.ToArray()), tri_n2 = Pin(n2.ToArray()), tri_n3 = Pin(n3.ToArray()), tri_material = Pin(tm.ToArray()),
                num_meshes = mf.Count, mesh_first = Pin(mf.ToArray()), mesh_count = Pin(mc.ToArray()),
                tri_t1 = Pin(t1.ToArray()), tri_t2 = Pin(t2.ToArray()), tri_t3 = Pin(t3.ToArray()),
                env_texture = Tid(Scene.Texture), env_texture_angle = Scene.TextureAngle,
            };
            d.env_color[0] = Scene.Color.r; d.env_color[1] = Scene.Color.g; d.env_color[2] = Scene.Color.b;
            d.num_textures = texs.Count; d.textures = Pin(texs.ToArray());
            d.num_sdf_nodes = sdfNodes.Count; d.sdf_nodes = Pin(sdfNodes.ToArray()); d.sdf_children = Pin(sdfKids.ToArray());
            d.num_sdf_shapes = sdfShapes.Count; d.sdf_shapes = Pin(sdfShapes.ToArray());
            d.num_volumes = vols.Count; d.volumes = Pin(vols.ToArray());
            d.num_transformed = xfs.Count; d.transformed = Pin(xfs.ToArray());
            try { PtHip.Check(PtHip.pt_upload_scene(ctx, ref d), "pt_upload_scene"); }
            finally { foreach (var g in pins) g.Free(); pins.Clear(); }   // arrays are copied during the call
            uploaded = true;
        }

        unsafe PtHip.pt_camera Cam()
        {
            var c = new PtHip.pt_camera { m = Camera.m, focal_distance = Camera.focalDistance, aperture_radius = Camera.apertureRadius };
            c.p[0] = (float)Camera.p.X; c.p[1] = (float)Camera.p.Y; c.p[2] = (float)Camera.p.Z;
            c.u[0] = (float)Camera.u.X; c.u[1] = (float)Camera.u.Y; c.u[2] = (float)Camera.u.Z;
            c.v[0] = (float)Camera.v.X; c.v[1] = (float)Camera.v.Y; c.v[2] = (float)Camera.v.Z;
            c.w[0] = (float)Camera.w.X; c.w[1] = (float)Camera.w.Y; c.w[2] = (float)Camera.w.Z;
            return c;
        }

        /// <summary>One Renderer.RenderParallel pass on the GPU (Renderer.cs:199-338).</summary>
        public void RenderParallel() => Pass(0);

        /// <summary>One Renderer.Render pass (Renderer.cs:80-198, the NumCPU == 1 twin): the same main
        /// samples, then per pixel its adaptive and firefly samples (PT_PASS_SERIAL).</summary>
        public void Render() => Pass(PtHip.PT_PASS_SERIAL);

        /// <summary>k consecutive RenderParallel passes in one call (pt_pass_params.passes): the Buffer
        /// k RenderParallel() calls leave, bit for bit; plain passes run as one GPU batch, so a rank's
        /// tile share fills the device like a whole frame.  (IterativeRender keeps one pass per PNG.)</summary>
        public void RenderPasses(int k) => Pass(0, k);

        void Pass(int flags, int passes = 1)
        {
            if (!uploaded) Upload();
            var cam = Cam();
            var smp = new PtHip.pt_sampler { first_hit_samples = firstHit, max_bounces = maxBounces,
                direct_lighting = directLighting ? 1 : 0, soft_shadows = softShadows ? 1 : 0,
                light_mode = (int)Sampler.LightMode, specular_mode = (int)Sampler.SpecularMode };
            var pass = new PtHip.pt_pass_params { spp = SamplesPerPixel, stratified = StratifiedSampling ? 1 : 0,
                seed = Seed, pass_index = (uint)(this.pass + 1), adaptive_samples = AdaptiveSamples,
                firefly_samples = FireflySamples, flags = flags, passes = passes };
            this.pass += passes;
            GCHandle tiles = default;
            if (Tiles != null)
            {
                tiles = GCHandle.Alloc(Tiles, GCHandleType.Pinned);
                pass.num_tiles = Tiles.Length; pass.tiles = tiles.AddrOfPinnedObject();
            }
            try { PtHip.Check(PtHip.pt_render_pass(ctx, ref cam, ref smp, ref pass), "pt_render_pass"); }
            finally { if (tiles.IsAllocated) tiles.Free(); }
        }

        /// <summary>Resume: load a saved Buffer (e.g. Renderer.PBuffer of an earlier IterativeRender) into
        /// the GPU's Welford state; later passes keep accumulating into it (Renderer.cs:702-765).  `passesDone`
        /// continues the pass numbering the random streams are keyed by.</summary>
        public void LoadBuffer(Buffer b, int passesDone)
        {
            int P = W * H;
            var m = new double[3 * P]; var v = new double[3 * P]; var n = new int[P];
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++)
                {
                    int i = y * W + x; var px = b.Pixels[(x, y)];
                    n[i] = px.Samples;
                    m[3 * i] = px.M.r; m[3 * i + 1] = px.M.g; m[3 * i + 2] = px.M.b;
                    v[3 * i] = px.V.r; v[3 * i + 1] = px.V.g; v[3 * i + 2] = px.V.b;
                }
            PtHip.Check(PtHip.pt_write_buffer(ctx, m, v, n), "pt_write_buffer");
            pass = passesDone;
        }

        /// <summary>The Buffer pixels of 32x32 tiles, packed row-major inside each tile (pt_read_tiles):
        /// m, v [tiles][32][32][3], n [tiles][32][32].  With WriteTiles, a host that moves Buffers over
        /// its own transport assembles a sharded frame (pt_comm_gather's protocol).</summary>
        public (double[] m, double[] v, int[] n) ReadTiles(int[] tiles)
        {
            var m = new double[tiles.Length * 3072]; var v = new double[tiles.Length * 3072]; var n = new int[tiles.Length * 1024];
            PtHip.Check(PtHip.pt_read_tiles(ctx, tiles, tiles.Length, m, v, n), "pt_read_tiles");
            return (m, v, n);
        }

        public void WriteTiles(int[] tiles, double[] m, double[] v, int[] n) =>
            PtHip.Check(PtHip.pt_write_tiles(ctx, tiles, tiles.Length, m, v, n), "pt_write_tiles");

        /// <summary>Copy the HBM Welford state into Renderer.PBuffer's Pixel objects (Buffer.cs:18-58).</summary>
        public void ReadBuffer()
        {
            int P = W * H;
            var m = new double[3 * P]; var v = new double[3 * P]; var n = new int[P];
            PtHip.Check(PtHip.pt_read_buffer(ctx, m, v, n), "pt_read_buffer");
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++)
                {
                    int i = y * W + x;
                    Renderer.PBuffer.Pixels[(x, y)] = new Pixel(n[i], new Colour(m[3 * i], m[3 * i + 1], m[3 * i + 2]),
                                                                 new Colour(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
                }
        }

        /// <summary>Renderer.IterativeRender (Renderer.cs:702-765): N passes, a PNG after each.</summary>
        public SKBitmap IterativeRender(string pathTemplate, int iter)
        {
            SKBitmap colour = null;
            for (int i = 1; i <= iter; i++)
            {
                Console.WriteLine("Iteration " + i + " of " + iter);
                if (NumCPU == 1) Render(); else RenderParallel();   // Renderer.cs:712-719
                if (DeviceImages) colour = ReadBitmap(Channel.ColorChannel);
                else
                {
                    ReadBuffer();
                    colour = Renderer.PBuffer.Image(Channel.ColorChannel);
                }
                using (var stream = System.IO.File.OpenWrite(string.Format(pathTemplate, i)))
                    colour.Encode(SKEncodedImageFormat.Png, 100).SaveTo(stream);
                if (Denoise) colour = WriteDenoiseOutputs(pathTemplate);
            }
            if (DeviceImages) ReadBuffer();   // Renderer.PBuffer once, after the last pass
            return colour;
        }

        /// <summary>Filter the Buffer as it stands into the context's denoised result (pt_denoise); the Buffer
        /// and the pass state are unchanged.  Returns the device time of its kernels in ms.</summary>
        public double DenoiseBuffer()
        {
            if (DenoiseGuided)
            {
                if (!haveFeatures) RenderFeatures();   // once: the features do not change with the passes
                var g = new PtHip.pt_denoise_guided_params { iterations = DenoiseIterations, reserved = 0, sigma_colour = DenoiseSigmaColour,
                    sigma_normal = DenoiseSigmaNormal, sigma_albedo = DenoiseSigmaAlbedo, sigma_depth = DenoiseSigmaDepth };
                PtHip.Check(PtHip.pt_denoise_guided(ctx, ref g, out double gms), "pt_denoise_guided");
                return gms;
            }
            var p = new PtHip.pt_denoise_params { iterations = DenoiseIterations, reserved = 0, sigma_colour = DenoiseSigmaColour };
            PtHip.Check(PtHip.pt_denoise(ctx, ref p, out double ms), "pt_denoise");
            return ms;
        }

        /// <summary>AccumulateTemporal's parameters: the samples the history may weigh at most (0..2^20) and the relative
        /// depth tolerance (0 = off).  Design defaults, not tuned values.</summary>
        public int TemporalMaxHistory = 32;
        public double TemporalSigmaDepth = 0.1;

        /// <summary>Record the camera and the geometry as the device holds it as "the previous frame" (pt_motion_snapshot).</summary>
        public void MotionSnapshot()
        {
            var cam = Cam();
            PtHip.Check(PtHip.pt_motion_snapshot(ctx, ref cam), "pt_motion_snapshot");
        }

        /// <summary>One ray through each pixel's centre and where its hit point was in the snapshot's frame
        /// (pt_render_motion).  Returns the device time of the kernel in ms.</summary>
        public double RenderMotion()
        {
            var cam = Cam();
            PtHip.Check(PtHip.pt_render_motion(ctx, ref cam, out double ms), "pt_render_motion");
            return ms;
        }

        /// <summary>One array of the last RenderMotion (pt_read_motion; what: PtHip.PT_MOTION_*): int[W*H] for the _I32
        /// arrays, double[W*H] for the _F64 ones, double[W*H*2] for PT_MOTION_PREV_XY_F64.</summary>
        public Array Motion(int what)
        {
            bool f64 = what == PtHip.PT_MOTION_DEPTH_F64 || what == PtHip.PT_MOTION_PREV_XY_F64 || what == PtHip.PT_MOTION_PREV_DEPTH_F64;
            int n = W * H * (what == PtHip.PT_MOTION_PREV_XY_F64 ? 2 : 1);
            Array a = f64 ? new double[n] : new int[n];
            var pin = GCHandle.Alloc(a, GCHandleType.Pinned);
            try { PtHip.Check(PtHip.pt_read_motion(ctx, what, pin.AddrOfPinnedObject()), "pt_read_motion"); }
            finally { pin.Free(); }
            return a;
        }

        /// <summary>Merge the history into the Buffer's statistics through the last RenderMotion
        /// (pt_accumulate_temporal); the Buffer is unchanged.  Returns the device time of the kernel in ms.</summary>
        public double AccumulateTemporal()
        {
            var p = new PtHip.pt_temporal_params { max_history = TemporalMaxHistory, reserved = 0, sigma_depth = TemporalSigmaDepth };
            PtHip.Check(PtHip.pt_accumulate_temporal(ctx, ref p, out double ms), "pt_accumulate_temporal");
            return ms;
        }

        /// <summary>The last AccumulateTemporal's result (pt_read_temporal): M, V [W*H*3], N, status [W*H].</summary>
        public void Temporal(double[] m, double[] v, int[] n, int[] status)
        {
            PtHip.Check(PtHip.pt_read_temporal(ctx, m, v, n, status), "pt_read_temporal");
        }

        /// <summary>DenoiseBuffer on the temporal result instead of the Buffer (pt_denoise_temporal).</summary>
        public unsafe double DenoiseTemporal()
        {
            double ms;
            if (DenoiseGuided)
            {
                if (!haveFeatures) RenderFeatures();
                var g = new PtHip.pt_denoise_guided_params { iterations = DenoiseIterations, reserved = 0, sigma_colour = DenoiseSigmaColour,
                    sigma_normal = DenoiseSigmaNormal, sigma_albedo = DenoiseSigmaAlbedo, sigma_depth = DenoiseSigmaDepth };
                PtHip.Check(PtHip.pt_denoise_temporal(ctx, IntPtr.Zero, (IntPtr)(&g), out ms), "pt_denoise_temporal");
                return ms;
            }
            var p = new PtHip.pt_denoise_params { iterations = DenoiseIterations, reserved = 0, sigma_colour = DenoiseSigmaColour };
            PtHip.Check(PtHip.pt_denoise_temporal(ctx, (IntPtr)(&p), IntPtr.Zero, out ms), "pt_denoise_temporal");
            return ms;
        }

        /// <summary>Drop the history and the temporal and motion results, keep the snapshot (pt_reset_temporal): after a
        /// cut, or after a change of materials or lights, which nothing detects.</summary>
        public void ResetTemporal() { PtHip.Check(PtHip.pt_reset_temporal(ctx), "pt_reset_temporal"); }

        /// <summary>The temporal half of one animated frame, after its passes.</summary>
        public void TemporalFrame()
        {
            RenderMotion();
            AccumulateTemporal();
            MotionSnapshot();
        }

        /// <summary>New vertex positions (and optionally normals, all three or none) for every triangle of the
        /// uploaded scene, [n * 3] floats in the upload's order (pt_update_triangles): the triangle BVH is
        /// refitted on the device, nothing is rebuilt.  The caller keeps its own scene in step.  Returns the
        /// device time of the kernels in ms.</summary>
        public double UpdateTriangles(float[] v1, float[] v2, float[] v3, float[] n1 = null, float[] n2 = null, float[] n3 = null)
        {
            if (!uploaded) Upload();
            PtHip.Check(PtHip.pt_update_triangles(ctx, v1.Length / 3, v1, v2, v3, n1, n2, n3, out double ms), "pt_update_triangles");
            return ms;
        }

        /// <summary>UpdateTriangles with the normals derived on the device from the new positions
        /// (pt_update_triangles_normals): mode PtHip.PT_NORMALS_FACE, every corner the triangle's face normal, or
        /// PtHip.PT_NORMALS_SMOOTH, Mesh.SmoothNormals on each mesh of the scene.  Returns the device time of
        /// the kernels in ms; ReadTriNormals returns what was computed.</summary>
        public double UpdateTrianglesNormals(float[] v1, float[] v2, float[] v3, int mode)
        {
            if (!uploaded) Upload();
            PtHip.Check(PtHip.pt_update_triangles_normals(ctx, v1.Length / 3, v1, v2, v3, mode, out double ms), "pt_update_triangles_normals");
            return ms;
        }

        /// <summary>The normals the uploaded scene holds on the device now (pt_read_tri_normals): [n * 3] floats
        /// each, in the upload's triangle order.</summary>
        public (float[] n1, float[] n2, float[] n3) ReadTriNormals(int numTriangles)
        {
            if (!uploaded) Upload();
            var n1 = new float[numTriangles * 3];
            var n2 = new float[numTriangles * 3];
            var n3 = new float[numTriangles * 3];
            PtHip.Check(PtHip.pt_read_tri_normals(ctx, n1, n2, n3), "pt_read_tri_normals");
            return (n1, n2, n3);
        }

        /// <summary>The context's triangle BVH as it stands on the device (pt_read_tri_bvh): 32 words per node,
        /// leaf chunk and triangle record, and the root box.</summary>
        public (uint[] nodes, uint[] chunks, uint[] records, float[] box) ReadTriBvh()
        {
            if (!uploaded) Upload();
            var counts = new long[3];
            PtHip.Check(PtHip.pt_read_tri_bvh(ctx, counts, null, null, null, null), "pt_read_tri_bvh");
            var nodes = new uint[counts[0] * 32];
            var chunks = new uint[counts[1] * 32];
            var records = new uint[counts[2] * 32];
            var box = new float[6];
            PtHip.Check(PtHip.pt_read_tri_bvh(ctx, counts, nodes, chunks, records, box), "pt_read_tri_bvh");
            return (nodes, chunks, records, box);
        }

        /// <summary>New parameters for the spheres, cubes and transformed shapes of the uploaded scene, in the
        /// upload's order (pt_update_shapes): centres [n * 3] with optional radii [n], cube corners [n * 3] each,
        /// matrices and inverses [n * 16] row-major; a null group stays.  The analytic BVH is refitted on the
        /// device, nothing is rebuilt.  The caller keeps its own scene in step.  Returns the device time of the
        /// kernels in ms.</summary>
        public double UpdateShapes(float[] sphereCenter = null, double[] sphereRadius = null, float[] cubeMin = null,
                                   float[] cubeMax = null, double[] matrices = null, double[] inverses = null)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            IntPtr PinHeld(Array a)
            {
                if (a == null) return IntPtr.Zero;
                var h = GCHandle.Alloc(a, GCHandleType.Pinned);
                held.Add(h);
                return h.AddrOfPinnedObject();
            }
            try
            {
                var u = new PtHip.pt_shape_update
                {
                    num_spheres = sphereCenter == null ? 0 : sphereCenter.Length / 3,
                    num_cubes = cubeMin == null ? 0 : cubeMin.Length / 3,
                    num_transformed = matrices == null ? 0 : matrices.Length / 16,
                    reserved = 0,
                    sphere_center = PinHeld(sphereCenter), sphere_radius = PinHeld(sphereRadius),
                    cube_min = PinHeld(cubeMin), cube_max = PinHeld(cubeMax),
                    xform_matrix = PinHeld(matrices), xform_inverse = PinHeld(inverses),
                };
                PtHip.Check(PtHip.pt_update_shapes(ctx, ref u, out double ms), "pt_update_shapes");
                return ms;
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>UpdateTriangles / UpdateTrianglesNormals for a scene that may hold instanced meshes
        /// (pt_update_meshes; those two refuse such a scene): new positions for every triangle, instanced meshes'
        /// included, the normals given (all three), kept (all null) or derived (normalsMode PtHip.PT_NORMALS_FACE
        /// or PT_NORMALS_SMOOTH).  Every BLAS is refitted on the device, the instances' boxes and the analytic BVH
        /// follow; nothing is rebuilt.  Returns the device time of the kernels in ms.</summary>
        public double UpdateMeshes(float[] v1, float[] v2, float[] v3, float[] n1 = null, float[] n2 = null, float[] n3 = null,
                                   int normalsMode = 0)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            IntPtr PinHeld(Array a)
            {
                if (a == null) return IntPtr.Zero;
                var h = GCHandle.Alloc(a, GCHandleType.Pinned);
                held.Add(h);
                return h.AddrOfPinnedObject();
            }
            try
            {
                var u = new PtHip.pt_mesh_update
                {
                    num_triangles = v1.Length / 3, normals_mode = normalsMode,
                    v1 = PinHeld(v1), v2 = PinHeld(v2), v3 = PinHeld(v3), n1 = PinHeld(n1), n2 = PinHeld(n2), n3 = PinHeld(n3),
                };
                PtHip.Check(PtHip.pt_update_meshes(ctx, ref u, out double ms), "pt_update_meshes");
                return ms;
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>Installs the rest pose PoseMeshes poses from (pt_set_rest_pose): positions and normals of every
        /// triangle of the uploaded scene, kept on the device until the next upload.</summary>
        public void SetRestPose(float[] v1, float[] v2, float[] v3, float[] n1, float[] n2, float[] n3)
        {
            if (!uploaded) Upload();
            PtHip.Check(PtHip.pt_set_rest_pose(ctx, v1.Length / 3, v1, v2, v3, n1, n2, n3), "pt_set_rest_pose");
        }

        /// <summary>Mesh.Transform(matrices[j]) of every mesh j of the uploaded scene on the device, from the rest pose
        /// SetRestPose installed (pt_pose_meshes): matrices holds 16 doubles per mesh, row-major, in the scene's mesh
        /// order; mask (optional, one int per mesh) is 0 for a mesh that takes its rest values.  normalsMode 0
        /// transforms the rest normals as Mesh.Transform does, PtHip.PT_NORMALS_FACE or PT_NORMALS_SMOOTH derives
        /// them from the posed positions.  The BVHs, the instances' boxes and the lights follow as in UpdateMeshes.
        /// Returns the device time of the kernels in ms.</summary>
        public double PoseMeshes(double[] matrices, int[] mask = null, int normalsMode = 0)
        {
            if (!uploaded) Upload();
            var hm = GCHandle.Alloc(matrices, GCHandleType.Pinned);
            var hk = mask == null ? default(GCHandle) : GCHandle.Alloc(mask, GCHandleType.Pinned);
            try
            {
                var u = new PtHip.pt_mesh_pose
                {
                    num_meshes = matrices.Length / 16, normals_mode = normalsMode,
                    matrices = hm.AddrOfPinnedObject(), mesh_mask = mask == null ? IntPtr.Zero : hk.AddrOfPinnedObject(),
                };
                PtHip.Check(PtHip.pt_pose_meshes(ctx, ref u, out double ms), "pt_pose_meshes");
                return ms;
            }
            finally
            {
                hm.Free();
                if (mask != null) hk.Free();
            }
        }

        /// <summary>Installs the skin SkinMeshes blends with (pt_set_skin): bones[c] and weights[c] hold four bone
        /// indices and four weights per triangle for corner c + 1 of every triangle of the uploaded scene; a weight of
        /// 0 makes its influence dead.  Kept on the device until the next upload.</summary>
        public void SetSkin(int[][] bones, float[][] weights, int numBones)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            try
            {
                IntPtr Pin(object a) { var h = GCHandle.Alloc(a, GCHandleType.Pinned); held.Add(h); return h.AddrOfPinnedObject(); }
                var d = new PtHip.pt_skin_desc
                {
                    num_triangles = bones[0].Length / PtHip.PT_SKIN_INFLUENCES, num_bones = numBones,
                    bone1 = Pin(bones[0]), bone2 = Pin(bones[1]), bone3 = Pin(bones[2]),
                    weight1 = Pin(weights[0]), weight2 = Pin(weights[1]), weight3 = Pin(weights[2]),
                };
                PtHip.Check(PtHip.pt_set_skin(ctx, ref d), "pt_set_skin");
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>Linear blend skinning of every mesh of the uploaded scene on the device, from the rest pose
        /// SetRestPose installed and the skin SetSkin installed (pt_skin_meshes): matrices holds 16 doubles per bone,
        /// row-major.  normalsMode 0 blends the transformed rest normals, PtHip.PT_NORMALS_FACE or PT_NORMALS_SMOOTH
        /// derives them from the skinned positions.  The BVHs, the instances' boxes and the lights follow as in
        /// UpdateMeshes; ReadPose returns the skinned arrays.  Returns the device time of the kernels in ms.</summary>
        public double SkinMeshes(double[] matrices, int normalsMode = 0)
        {
            if (!uploaded) Upload();
            var hm = GCHandle.Alloc(matrices, GCHandleType.Pinned);
            try
            {
                var u = new PtHip.pt_mesh_skin { num_bones = matrices.Length / 16, normals_mode = normalsMode, matrices = hm.AddrOfPinnedObject() };
                PtHip.Check(PtHip.pt_skin_meshes(ctx, ref u, out double ms), "pt_skin_meshes");
                return ms;
            }
            finally
            {
                hm.Free();
            }
        }

        /// <summary>Installs the morph targets MorphMeshes adds to the rest pose (pt_set_morph): target t owns the
        /// deltas targetFirst[t] .. targetFirst[t + 1] - 1; delta i moves corner corner[i] = 3 * triangle + c by
        /// dpos[3 i ..] and, when dnrm is not null, its normal by dnrm[3 i ..].  Kept on the device until the next
        /// upload.</summary>
        public void SetMorph(int numTriangles, long[] targetFirst, int[] corner, float[] dpos, float[] dnrm = null)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            try
            {
                IntPtr Pin(object a) { var h = GCHandle.Alloc(a, GCHandleType.Pinned); held.Add(h); return h.AddrOfPinnedObject(); }
                var d = new PtHip.pt_morph_desc
                {
                    num_triangles = numTriangles, num_targets = targetFirst.Length - 1,
                    target_first = Pin(targetFirst), corner = Pin(corner), dpos = Pin(dpos),
                    dnrm = dnrm == null ? IntPtr.Zero : Pin(dnrm),
                };
                PtHip.Check(PtHip.pt_set_morph(ctx, ref d), "pt_set_morph");
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>Morphs every mesh of the uploaded scene on the device, from the rest pose SetRestPose installed and
        /// the targets SetMorph installed (pt_morph_meshes): weights holds one float per target, 0 makes it dead.
        /// normalsMode 0 adds the normal deltas to the rest normals, PtHip.PT_NORMALS_FACE or PT_NORMALS_SMOOTH derives
        /// them from the morphed positions.  skinMatrices (16 doubles per bone of the skin SetSkin installed, or null)
        /// skins the morphed pose as SkinMeshes skins the rest pose.  ReadPose returns the arrays.  Returns the device
        /// time of the kernels in ms.</summary>
        public double MorphMeshes(float[] weights, int normalsMode = 0, double[] skinMatrices = null)
        {
            if (!uploaded) Upload();
            var hw = GCHandle.Alloc(weights, GCHandleType.Pinned);
            var hm = skinMatrices == null ? default(GCHandle) : GCHandle.Alloc(skinMatrices, GCHandleType.Pinned);
            try
            {
                var u = new PtHip.pt_mesh_morph
                {
                    num_targets = weights.Length, normals_mode = normalsMode, num_bones = skinMatrices == null ? 0 : skinMatrices.Length / 16,
                    weights = hw.AddrOfPinnedObject(), skin_matrices = skinMatrices == null ? IntPtr.Zero : hm.AddrOfPinnedObject(),
                };
                PtHip.Check(PtHip.pt_morph_meshes(ctx, ref u, out double ms), "pt_morph_meshes");
                return ms;
            }
            finally
            {
                hw.Free();
                if (skinMatrices != null) hm.Free();
            }
        }

        /// <summary>The six arrays the last PoseMeshes, SkinMeshes or MorphMeshes left on the device (pt_read_pose), 3 floats per triangle each:
        /// v1, v2, v3, n1, n2, n3, derived normals included.</summary>
        public float[][] ReadPose(int numTriangles)
        {
            var a = new float[6][];
            for (int k = 0; k < 6; k++) a[k] = new float[numTriangles * 3];
            PtHip.Check(PtHip.pt_read_pose(ctx, a[0], a[1], a[2], a[3], a[4], a[5]), "pt_read_pose");
            return a;
        }

        /// <summary>UpdateMeshes that also re-sorts the world triangle BVH on the device into a balanced median tree for
        /// the new positions (pt_rebuild_meshes), for a mesh deformed far from the pose its tree was built for.  A scene
        /// with an instanced mesh is refused.  Returns the device time of the kernels in ms.</summary>
        public double RebuildMeshes(float[] v1, float[] v2, float[] v3, float[] n1 = null, float[] n2 = null, float[] n3 = null,
                                    int normalsMode = 0)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            IntPtr PinHeld(Array a)
            {
                if (a == null) return IntPtr.Zero;
                var h = GCHandle.Alloc(a, GCHandleType.Pinned);
                held.Add(h);
                return h.AddrOfPinnedObject();
            }
            try
            {
                var u = new PtHip.pt_mesh_update
                {
                    num_triangles = v1.Length / 3, normals_mode = normalsMode,
                    v1 = PinHeld(v1), v2 = PinHeld(v2), v3 = PinHeld(v3), n1 = PinHeld(n1), n2 = PinHeld(n2), n3 = PinHeld(n3),
                };
                PtHip.Check(PtHip.pt_rebuild_meshes(ctx, ref u, out double ms), "pt_rebuild_meshes");
                return ms;
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>RebuildMeshes from the pose or skin the last PoseMeshes or SkinMeshes left staged on the device: nothing is copied.</summary>
        public double RebuildMeshes()
        {
            PtHip.Check(PtHip.pt_rebuild_meshes(ctx, IntPtr.Zero, out double ms), "pt_rebuild_meshes");
            return ms;
        }

        /// <summary>UpdateMeshes that also re-sorts every instanced mesh's BLAS on the device into a balanced median
        /// tree for the new positions (pt_rebuild_blas), and with PT_REBUILD_WORLD in <paramref name="what"/> (0: both)
        /// the world triangle BVH as RebuildMeshes does.  A BLAS whose balanced tree needs more nodes than the upload
        /// gave it is refitted instead.  Returns the device time of the kernels in ms.</summary>
        public double RebuildBlas(float[] v1, float[] v2, float[] v3, float[] n1 = null, float[] n2 = null, float[] n3 = null,
                                  int normalsMode = 0, int what = 0)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            IntPtr PinHeld(Array a)
            {
                if (a == null) return IntPtr.Zero;
                var h = GCHandle.Alloc(a, GCHandleType.Pinned);
                held.Add(h);
                return h.AddrOfPinnedObject();
            }
            try
            {
                var u = new PtHip.pt_mesh_update
                {
                    num_triangles = v1.Length / 3, normals_mode = normalsMode,
                    v1 = PinHeld(v1), v2 = PinHeld(v2), v3 = PinHeld(v3), n1 = PinHeld(n1), n2 = PinHeld(n2), n3 = PinHeld(n3),
                };
                PtHip.Check(PtHip.pt_rebuild_blas(ctx, ref u, what, out double ms), "pt_rebuild_blas");
                return ms;
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>RebuildBlas from the pose or skin the last PoseMeshes or SkinMeshes left staged on the device: nothing is copied.</summary>
        public double RebuildBlas(int what = 0)
        {
            PtHip.Check(PtHip.pt_rebuild_blas(ctx, IntPtr.Zero, what, out double ms), "pt_rebuild_blas");
            return ms;
        }

        /// <summary>The surface-area cost of every BLAS as it stands (pt_blas_cost): per BLAS the inner cost and the
        /// leaf cost relative to its root box's area, and that area.  Its growth since the upload tells when
        /// RebuildBlas pays.</summary>
        public double[] BlasCost()
        {
            if (!uploaded) Upload();
            var counts = new long[3];
            PtHip.Check(PtHip.pt_read_blas(ctx, counts, null, null, null, null, null), "pt_read_blas");
            var o = new double[Math.Max(1, counts[0] * 3)];
            PtHip.Check(PtHip.pt_blas_cost(ctx, (int)counts[0], o), "pt_blas_cost");
            return o;
        }

        /// <summary>New voxels and new iso-windows for the Volumes of the uploaded scene, in the upload's volume order
        /// (pt_update_volumes): data[i] holds W*H*D doubles (Data[x + y*W + z*W*H]) or is null (volume i keeps its
        /// voxels); windows[i] holds the volume's uploaded number of windows with new lo and hi (the materials must be
        /// the uploaded ones) or is null.  Either array may be null.  The volumes' derived tables are rebuilt on the
        /// device; a volume given windows only sends no voxels.  An edit that would make a Volume start or stop being
        /// a light is refused (PT_ERR_UNSUPPORTED): upload the scene again.  Returns the device time of the kernels in
        /// ms.</summary>
        public double UpdateVolumes(int numVolumes, double[][] data = null, PtHip.pt_volume_window[][] windows = null)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            IntPtr PinHeld(Array a)
            {
                if (a == null) return IntPtr.Zero;
                var h = GCHandle.Alloc(a, GCHandleType.Pinned);
                held.Add(h);
                return h.AddrOfPinnedObject();
            }
            try
            {
                // the pointer arrays and every array they name stay pinned for the call
                IntPtr[] dp = data == null ? null : new IntPtr[Math.Max(1, numVolumes)];
                IntPtr[] wp = windows == null ? null : new IntPtr[Math.Max(1, numVolumes)];
                for (int i = 0; i < numVolumes; i++)
                {
                    if (dp != null && i < data.Length) dp[i] = PinHeld(data[i]);
                    if (wp != null && i < windows.Length) wp[i] = PinHeld(windows[i]);
                }
                var u = new PtHip.pt_volume_update { num_volumes = numVolumes, data = PinHeld(dp), windows = PinHeld(wp) };
                PtHip.Check(PtHip.pt_update_volumes(ctx, ref u, out double ms), "pt_update_volumes");
                return ms;
            }
            finally
            {
                foreach (var h in held) h.Free();
            }
        }

        /// <summary>New materials and a new environment for the uploaded scene (pt_update_materials): materials holds
        /// the scene's whole table in the upload's order, or is null (kept); with env the environment colour, texture
        /// slot (1-based, 0 = none) and angle are taken.  The lights and the routing flags follow on the device as at
        /// an upload: a shape whose material now emits becomes a light, one that no longer does stops being one.  No
        /// geometry is re-sent.  Returns 0: the call launches no kernel.</summary>
        public unsafe double UpdateMaterials(PtHip.pt_material[] materials, bool env = false, double[] envColor = null,
                                             int envTexture = 0, double envTextureAngle = 0)
        {
            if (!uploaded) Upload();
            var h = materials == null ? default : GCHandle.Alloc(materials, GCHandleType.Pinned);
            try
            {
                var u = new PtHip.pt_material_update
                {
                    num_materials = materials?.Length ?? 0,
                    flags = env ? PtHip.PT_LOOK_ENV : 0,
                    materials = materials == null ? IntPtr.Zero : h.AddrOfPinnedObject(),
                    env_texture = envTexture,
                    env_texture_angle = envTextureAngle
                };
                for (int k = 0; k < 3 && envColor != null; k++) u.env_color[k] = envColor[k];
                PtHip.Check(PtHip.pt_update_materials(ctx, ref u, out double ms), "pt_update_materials");
                return ms;
            }
            finally
            {
                if (materials != null) h.Free();
            }
        }

        /// <summary>New texels for the textures of the uploaded scene, in the upload's texture order
        /// (pt_update_textures): images[i] is null (texture i stays) or an image of the uploaded size whose data and
        /// lut the caller keeps pinned for the call.  The 8-bit formats are decoded on the device through lut.  Returns
        /// the device time of the decode kernels in ms.</summary>
        public double UpdateTextures(PtHip.pt_texture_image?[] images)
        {
            if (!uploaded) Upload();
            var held = new List<GCHandle>();
            try
            {
                var ptrs = new IntPtr[Math.Max(1, images.Length)];
                for (int i = 0; i < images.Length; i++)
                {
                    if (images[i] == null) continue;
                    var one = new[] { images[i].Value };
                    var hh = GCHandle.Alloc(one, GCHandleType.Pinned);
                    held.Add(hh);
                    ptrs[i] = hh.AddrOfPinnedObject();
                }
                var hp = GCHandle.Alloc(ptrs, GCHandleType.Pinned);
                held.Add(hp);
                var u = new PtHip.pt_texture_update { num_textures = images.Length, images = hp.AddrOfPinnedObject() };
                PtHip.Check(PtHip.pt_update_textures(ctx, ref u, out double ms), "pt_update_textures");
                return ms;
            }
            finally
            {
                foreach (var hh in held) hh.Free();
            }
        }

        /// <summary>The hits of n rays with their identity and Hit.Info (pt_intersect_hits).</summary>
        public sealed class Hits
        {
            public double[] T, Albedo, Gloss;
            public int[] Kind, Index, Prim, Shape, Inside, Material;
            public float[] Position, Normal;
        }

        /// <summary>Scene.Intersect of n rays ([n][3] origins and directions) with what was hit and where: the kind,
        /// the index in the scene's own arrays, the source triangle, the Scene.Shapes slot and, with info, Hit.Info's
        /// position, normal, side, material and MaterialAt colour and gloss (without it the kernel skips Hit.Info and
        /// those arrays stay null).</summary>
        public Hits IntersectHits(float[] origins, float[] dirs, bool info = true, int flags = 0)
        {
            if (!uploaded) Upload();
            int n = origins.Length / 3;
            var h = new Hits { T = new double[n], Kind = new int[n], Index = new int[n], Prim = new int[n], Shape = new int[n] };
            if (info)
            {
                h.Position = new float[3 * n]; h.Normal = new float[3 * n]; h.Inside = new int[n]; h.Material = new int[n];
                h.Albedo = new double[3 * n]; h.Gloss = new double[n];
            }
            var pins = new List<GCHandle>();
            IntPtr Pin(Array a)
            {
                if (a == null) return IntPtr.Zero;
                pins.Add(GCHandle.Alloc(a, GCHandleType.Pinned));
                return pins[pins.Count - 1].AddrOfPinnedObject();
            }
            try
            {
                var a = new PtHip.pt_hit_arrays
                {
                    t = Pin(h.T), kind = Pin(h.Kind), index = Pin(h.Index), prim = Pin(h.Prim), shape = Pin(h.Shape),
                    position = Pin(h.Position), normal = Pin(h.Normal), inside = Pin(h.Inside), material = Pin(h.Material),
                    albedo = Pin(h.Albedo), gloss = Pin(h.Gloss),
                };
                PtHip.Check(PtHip.pt_intersect_hits(ctx, n, origins, dirs, flags, ref a), "pt_intersect_hits");
            }
            finally
            {
                foreach (var p in pins) p.Free();
            }
            return h;
        }

        /// <summary>The surface-area cost of the world triangle BVH as it stands (pt_tri_bvh_cost): inner cost and leaf
        /// cost relative to the root box's area, and that area.  Its growth since the upload tells when RebuildMeshes
        /// pays.</summary>
        public (double inner, double leaf, double rootArea) TriBvhCost()
        {
            if (!uploaded) Upload();
            var o = new double[3];
            PtHip.Check(PtHip.pt_tri_bvh_cost(ctx, o), "pt_tri_bvh_cost");
            return (o[0], o[1], o[2]);
        }

        /// <summary>The context's BLASes as they stand on the device (pt_read_blas): 4 ints per BLAS, 32 words per
        /// node, 12 words per triangle in recs and in shade, 6 floats per BLAS (the mesh's unpadded box).</summary>
        public (int[] blas, uint[] nodes, uint[] recs, uint[] shade, float[] innerBoxes) ReadBlas()
        {
            if (!uploaded) Upload();
            var counts = new long[3];
            PtHip.Check(PtHip.pt_read_blas(ctx, counts, null, null, null, null, null), "pt_read_blas");
            var blas = new int[counts[0] * 4];
            var nodes = new uint[counts[1] * 32];
            var recs = new uint[counts[2] * 12];
            var shade = new uint[counts[2] * 12];
            var boxes = new float[counts[0] * 6];
            PtHip.Check(PtHip.pt_read_blas(ctx, counts, blas, nodes, recs, shade, boxes), "pt_read_blas");
            return (blas, nodes, recs, shade, boxes);
        }

        /// <summary>The first-hit features of the whole frame (pt_render_features): one ray through each
        /// pixel's centre, the lens ignored.  The Buffer and the pass state are unchanged.  Returns the
        /// device time of the kernel in ms.</summary>
        public double RenderFeatures()
        {
            if (!uploaded) Upload();
            var cam = Cam();
            PtHip.Check(PtHip.pt_render_features(ctx, ref cam, out double ms), "pt_render_features");
            haveFeatures = true;
            return ms;
        }

        /// <summary>The context's features (pt_read_features), row-major: albedo [H][W][3], normal [H][W][3],
        /// depth [H][W] (1e9 on a miss), kind [H][W] (the pt_shape_kind hit, or -1), material [H][W] (or -1).</summary>
        public (double[] albedo, float[] normal, double[] depth, int[] kind, int[] material) ReadFeatures()
        {
            int P = W * H;
            var albedo = new double[3 * P]; var normal = new float[3 * P]; var depth = new double[P];
            var kind = new int[P]; var material = new int[P];
            void Read(int feature, Array dst)
            {
                var pin = GCHandle.Alloc(dst, GCHandleType.Pinned);
                try { PtHip.Check(PtHip.pt_read_features(ctx, feature, pin.AddrOfPinnedObject()), "pt_read_features"); }
                finally { pin.Free(); }
            }
            Read(PtHip.PT_FEATURE_ALBEDO_F64, albedo); Read(PtHip.PT_FEATURE_NORMAL_F32, normal);
            Read(PtHip.PT_FEATURE_DEPTH_F64, depth); Read(PtHip.PT_FEATURE_KIND_I32, kind);
            Read(PtHip.PT_FEATURE_MATERIAL_I32, material);
            return (albedo, normal, depth, kind, material);
        }

        /// <summary>The last DenoiseBuffer()'s colour, encoded as ReadBitmap(ColorChannel) encodes M.  A
        /// snapshot: later passes do not change it.</summary>
        public SKBitmap Denoised()
        {
            var bmp = new SKBitmap(new SKImageInfo(W, H, SKColorType.Rgba8888, SKAlphaType.Opaque));
            var px = new byte[W * H * 4];
            var pin = GCHandle.Alloc(px, GCHandleType.Pinned);
            try { PtHip.Check(PtHip.pt_read_denoised(ctx, PtHip.PT_DENOISED_RGBA8, pin.AddrOfPinnedObject()), "pt_read_denoised"); }
            finally { pin.Free(); }
            for (int y = 0; y < H; y++)   // row by row: a bitmap's RowBytes may exceed 4 W
                Marshal.Copy(px, y * W * 4, IntPtr.Add(bmp.GetPixels(), y * bmp.RowBytes), W * 4);
            return bmp;
        }

        /// <summary>The denoise step of Renderer.cs:731-761 on this context's Buffer: the Albedo and Normal
        /// channels and the denoised colour as PNG files beside the pass images; returns the denoised image.</summary>
        internal SKBitmap WriteDenoiseOutputs(string pathTemplate)
        {
            string dir = System.IO.Path.GetDirectoryName(pathTemplate) ?? "";
            void Save(SKBitmap b, string name)
            {
                using var s = System.IO.File.OpenWrite(System.IO.Path.Combine(dir, name));
                b.Encode(SKEncodedImageFormat.Png, 100).SaveTo(s);
            }
            Save(ReadBitmap(Channel.AlbedoChannel), "albedo_channel.png");
            Save(ReadBitmap(Channel.NormalChannel), "normal_channel.png");
            DenoiseBuffer();
            var denoised = Denoised();
            Save(denoised, "denoised_output.png");
            return denoised;
        }

        /// <summary>Buffer.Image(channel) (Buffer.cs:134-202) resolved on the device (pt_read_image): row-major
        /// [H][W][3] bytes, or [H][W][4] with A = 255 when rgba.  The Buffer is the context's as it stands: this
        /// renderer's tiles, or the whole frame on the root after a gather.</summary>
        public byte[] ReadImage(Channel channel, bool rgba)
        {
            var px = new byte[W * H * (rgba ? 4 : 3)];
            PtHip.Check(PtHip.pt_read_image(ctx, (int)channel, rgba ? PtHip.PT_IMAGE_RGBA8 : PtHip.PT_IMAGE_RGB8, px), "pt_read_image");
            return px;
        }

        /// <summary>ReadImage as the SKBitmap Buffer.Image returns (SKColor(r, g, b, 255), Buffer.cs:160).</summary>
        public SKBitmap ReadBitmap(Channel channel)
        {
            var px = ReadImage(channel, true);
            var bmp = new SKBitmap(new SKImageInfo(W, H, SKColorType.Rgba8888, SKAlphaType.Opaque));
            for (int y = 0; y < H; y++)   // row by row: a bitmap's RowBytes may exceed 4 W
                Marshal.Copy(px, y * W * 4, IntPtr.Add(bmp.GetPixels(), y * bmp.RowBytes), W * 4);
            return bmp;
        }

        public void Dispose() { if (ctx != IntPtr.Zero) { PtHip.pt_destroy(ctx); ctx = IntPtr.Zero; } }
    }

    /// <summary>One .NET process driving G GPUs (the reference's Renderer is one process on all cores,
    /// Renderer.cs:257-333): one HipRenderer per device drawing its interleaved tiles, one RCCL
    /// communicator over the G contexts (pt_comm_init_all), passes issued from G host threads at once
    /// (a firefly pass all-reduces its snapshot across the group), the Buffer gathered onto device 0
    /// (pt_comm_gather_all) and copied into Renderer.PBuffer.</summary>
    class HipRendererGroup : IDisposable
    {
        readonly HipRenderer[] parts;
        readonly IntPtr[] ctxs;

        HipRendererGroup(HipRenderer[] p)
        {
            parts = p;
            ctxs = Array.ConvertAll(p, r => r.ctx);
            // the ranks' tile lists must be disjoint: checked once, before any RCCL call
            var all = new System.Collections.Generic.List<int>();
            foreach (var r in p) if (r.Tiles != null) all.AddRange(r.Tiles);
            PtHip.Check(PtHip.pt_tile_lists_check(all.ToArray(), all.Count, ((p[0].Width + 31) / 32) * ((p[0].Height + 31) / 32)),
                        "pt_tile_lists_check");
            PtHip.Check(PtHip.pt_comm_init_all(ctxs, ctxs.Length), "pt_comm_init_all");
        }

        public static HipRendererGroup NewRenderer(Scene scene, Camera camera, DefaultSampler sampler, int firstHitSamples,
                                                   int maxBounces, int w, int h, int[] devices)
        {
            var p = new HipRenderer[devices.Length];
            for (int i = 0; i < devices.Length; i++)
            {
                p[i] = HipRenderer.NewRenderer(scene, camera, sampler, firstHitSamples, maxBounces, w, h, devices[i]);
                p[i].Tiles = HipRenderer.TilesForRank(w, h, i, devices.Length);
            }
            return new HipRendererGroup(p);
        }

        public int SamplesPerPixel { set { foreach (var r in parts) r.SamplesPerPixel = value; } }
        public int AdaptiveSamples { set { foreach (var r in parts) r.AdaptiveSamples = value; } }
        public int FireflySamples { set { foreach (var r in parts) r.FireflySamples = value; } }
        public bool StratifiedSampling { set { foreach (var r in parts) r.StratifiedSampling = value; } }
        public ulong Seed { set { foreach (var r in parts) r.Seed = value; } }
        public int NumCPU { get => parts[0].NumCPU; set { foreach (var r in parts) r.NumCPU = value; } }
        /// <summary>As HipRenderer.DeviceImages: gather, resolve on device 0, one ReadBuffer after the last pass.</summary>
        public bool DeviceImages = false;
        /// <summary>As HipRenderer.Denoise: after each pass' gather device 0 holds the whole frame and denoises it.</summary>
        public bool Denoise = false;
        public int DenoiseIterations { set { parts[0].DenoiseIterations = value; } }
        public double DenoiseSigmaColour { set { parts[0].DenoiseSigmaColour = value; } }
        /// <summary>As HipRenderer.DenoiseGuided: device 0 renders the whole frame's features and filters with them.</summary>
        public bool DenoiseGuided { set { parts[0].DenoiseGuided = value; } }

        /// <summary>One RenderParallel pass on every GPU, one host thread per context.</summary>
        public void RenderParallel() => Parallel.For(0, parts.Length, new ParallelOptions { MaxDegreeOfParallelism = parts.Length },
                                                     i => parts[i].RenderParallel());

        /// <summary>One Render pass (the NumCPU == 1 twin, Renderer.cs:80-198) on every GPU: its extra
        /// phases decide per pixel, so the tile split renders exactly the one-GPU frame.</summary>
        public void Render() => Parallel.For(0, parts.Length, new ParallelOptions { MaxDegreeOfParallelism = parts.Length },
                                             i => parts[i].Render());

        /// <summary>Sum the ranks' disjoint tiles onto device 0 and copy them into Renderer.PBuffer.</summary>
        public void ReadBuffer()
        {
            Gather();
            parts[0].ReadBuffer();
        }

        // device 0 then holds every rank's tiles; its next pass clears the others' pixels again
        // (ptsharp_hip.h "Multi-GPU"), so the gather can follow every pass
        void Gather() => PtHip.Check(PtHip.pt_comm_gather_all(ctxs, ctxs.Length, 0), "pt_comm_gather_all");

        /// <summary>The whole frame's Buffer.Image(channel), gathered onto device 0 and resolved there.</summary>
        public byte[] ReadImage(Channel channel, bool rgba)
        {
            Gather();
            return parts[0].ReadImage(channel, rgba);
        }

        /// <summary>The whole frame gathered onto device 0, denoised there (pt_denoise) and read back.</summary>
        public SKBitmap Denoised()
        {
            Gather();
            parts[0].DenoiseBuffer();
            return parts[0].Denoised();
        }

        public SKBitmap IterativeRender(string pathTemplate, int iter)
        {
            SKBitmap colour = null;
            for (int i = 1; i <= iter; i++)
            {
                Console.WriteLine("Iteration " + i + " of " + iter);
                if (NumCPU == 1) Render(); else RenderParallel();   // Renderer.cs:712-719
                if (DeviceImages)
                {
                    Gather();   // device 0 holds the whole frame and resolves it
                    colour = parts[0].ReadBitmap(Channel.ColorChannel);
                }
                else
                {
                    ReadBuffer();
                    colour = Renderer.PBuffer.Image(Channel.ColorChannel);
                }
                using (var stream = System.IO.File.OpenWrite(string.Format(pathTemplate, i)))
                    colour.Encode(SKEncodedImageFormat.Png, 100).SaveTo(stream);
                if (Denoise) colour = parts[0].WriteDenoiseOutputs(pathTemplate);   // either path has gathered onto device 0
            }
            // Renderer.PBuffer once: the last pass' gather left the whole frame on device 0
            if (DeviceImages) { if (iter >= 1) parts[0].ReadBuffer(); else ReadBuffer(); }
            return colour;
        }

        public void Dispose() { foreach (var r in parts) r.Dispose(); }
    }

    /// <summary>OBJ.Load (OBJ.cs:11-165) parsed natively, same quirks; the Triangle[] is then
    /// built as Mesh.NewMesh does.  Replaces `OBJ.Load(path, material)` in Example.*.</summary>
    static class HipObj
    {
        static Vector V(float[] a, int i) => new Vector(a[3 * i], a[3 * i + 1], a[3 * i + 2]);

        internal static Mesh Load(string path, Material parent)
        {
            var rc = PtHip.pt_obj_load(path, out var md);
            if (rc != PtHip.PT_OK)
                throw new InvalidOperationException($"pt_obj_load failed ({rc}): {Marshal.PtrToStringAnsi(PtHip.pt_obj_last_error())}");
            try
            {
                int n = md.num_triangles;
                float[] Copy(IntPtr p) { var a = new float[3 * n]; if (n > 0) Marshal.Copy(p, a, 0, 3 * n); return a; }
                float[] v1 = Copy(md.v1), v2 = Copy(md.v2), v3 = Copy(md.v3), n1 = Copy(md.n1), n2 = Copy(md.n2),
                        n3 = Copy(md.n3), t1 = Copy(md.t1), t2 = Copy(md.t2), t3 = Copy(md.t3);
                var tris = new Triangle[n];
                for (int i = 0; i < n; i++)
                {
                    var t = new Triangle { V1 = V(v1, i), V2 = V(v2, i), V3 = V(v3, i), N1 = V(n1, i), N2 = V(n2, i),
                                           N3 = V(n3, i), T1 = V(t1, i), T2 = V(t2, i), T3 = V(t3, i), Material = parent };
                    tris[i] = t;   // FixNormals already applied by the loader
                }
                return Mesh.NewMesh(tris);
            }
            finally { PtHip.pt_mesh_free(ref md); }
        }
    }
}
