/*
 * ptsharp_hip.h — C-ABI of libptsharp_hip.so, the MI355X (gfx950) render hot path
 * that drops in for PTSharp's CPU `Renderer` (reference: akav/PTSharp).
 *
 * Boundary.  The C# side keeps scene construction (Example.*,
 * IShape/Material/Camera/Scene objects) and the `Buffer` output; it flattens the
 * scene once and calls these entry points through P/Invoke, following the same
 * create / commit / execute / release lifecycle and out-string error convention
 * the reference already uses for its only other native library, OIDN
 * (PTSharpCore/OIDN.cs:43-95, used at Renderer.cs:614-677).
 *
 * Which reference interface each entry point replaces:
 *   pt_create          Renderer.NewRenderer(scene,camera,sampler,w,h,mt)   Renderer.cs:35-56
 *                      (+ new Buffer(w,h)                                  Buffer.cs:67-80)
 *   pt_upload_scene    Scene.Compile() → Tree.NewTree / Mesh.Compile        Scene.cs:48-68, Tree.cs:22-29, Mesh.cs:45-57
 *                      (lights registered as in Scene.Add                  Scene.cs:29-38)
 *   pt_update_triangles (new) new vertex positions for the uploaded scene:  Example.cs:163-223 rebuilds the
 *   / pt_read_tri_bvh  the triangle BVH refitted on the device, no rebuild  scene for every frame of its loop
 *   pt_update_triangles_normals  the same with the normals derived on the   Triangle.FixNormals, Mesh.SmoothNormals
 *   / pt_read_tri_normals        device: face or smooth                     Triangle.cs:224-237, Mesh.cs:191-229
 *   pt_update_shapes   (new) new sphere, cube and TransformedShape          Example.cs:163-223 ("beads"): that loop
 *   / pt_read_shape_bvh parameters: the analytic BVH refitted on the device  moves 31,920 spheres, and no triangle
 *   pt_update_meshes   (new) pt_update_triangles / _normals for a scene with  Mesh.cs:88-120 (Mesh.BoundingBox),
 *   / pt_read_blas     instanced meshes too: their BLASes refitted on the   TransformedShape.cs:36-39
 *                      device, the instances' boxes and lights following
 *   pt_set_rest_pose   (new) Mesh.Transform(matrix) of every mesh of the      Mesh.cs:254-274 (Mesh.Transform; MoveTo
 *   / pt_pose_meshes   uploaded scene on the device, from a rest pose kept    and FitInside, Mesh.cs:237-252, end in it),
 *   / pt_read_pose     there: one matrix per mesh per call, then the refits   Matrix.cs:134-150
 *   pt_set_skin        (new) linear blend skinning of that rest pose on the   Matrix.MulPosition / MulDirection,
 *   / pt_skin_meshes   device: four bone indices and weights per corner sent  Matrix.cs:134-150 (the reference has no
 *   / pt_read_skin     once, one matrix per bone per call, then the refits    skinning)
 *   pt_set_morph       (new) morph targets (blend shapes) over that rest pose   (the reference has no morphing; the
 *   / pt_morph_meshes  on the device: sparse per-corner deltas sent once, one   arithmetic is fixed below)
 *   / pt_read_morph    weight per target per call, optionally the skin on top,
 *                      then the refits
 *   pt_rebuild_meshes  (new) pt_update_meshes that also re-sorts the world    Tree.NewTree, Tree.cs:22-29 (the reference
 *   / pt_tri_bvh_cost  triangle BVH into a balanced median tree on the device  builds a new tree for every frame's scene)
 *                      for the new positions; the SAH cost of the tree as it
 *                      stands, the host's trigger for "refit or rebuild"
 *   pt_rebuild_blas    (new) the same for every instanced mesh's BLAS, and    Mesh.Compile under TransformedShape,
 *   / pt_blas_cost     the cost of each BLAS as it stands                     Mesh.cs / TransformedShape.cs
 *   pt_update_volumes  (new) new voxels and iso-windows for the scene's         Volume.NewVolume, Volume.cs:48-71, and
 *   / pt_read_volume   Volumes: their derived tables rebuilt on the device      VolumeWindow, Volume.cs:8-19
 *   pt_update_materials (new) new materials and environment for the uploaded    Scene.Add, Scene.cs:29-38 (the lights
 *   / pt_read_materials scene: the lights and routing flags derived again        follow the emittances), Material.cs:8-62
 *   pt_update_textures (new) new texels for the scene's textures, 8-bit images   ColorTexture.NewTexture, Texture.cs:150-166,
 *   / pt_read_texture  decoded on the device through the host's 256-entry table  ITexture.Pow / MulScalar
 *   pt_render_pass    one Renderer.RenderParallel() pass                  Renderer.cs:199-338
 *                      (flag PT_PASS_SERIAL: one Renderer.Render() pass  Renderer.cs:80-198)
 *                      = spp × Camera.CastRay → DefaultSampler.Sample      Camera.cs:98-119, Sampler.cs:40-145,191-296
 *                        → Scene.Intersect → Tree/IShape.Intersect        Scene.cs:75-79, Tree.cs:31-128
 *                        → Buffer.AddSample (Welford)                     Buffer.cs:33-44,94-97
 *   pt_read_buffer     reading Renderer.PBuffer pixels {Samples, M, V}     Buffer.cs:18-58, Renderer.cs:20
 *   pt_read_image      Renderer.PBuffer.Image(channel), resolved on the    Buffer.cs:134-282
 *                      device to 8-bit RGB / RGBA
 *   pt_denoise /       Renderer.Denoise: the per-pass denoised image, by   Renderer.cs:731-761
 *   pt_read_denoised   a native variance-guided à-trous filter (not OIDN)
 *   pt_render_features Renderer.DenoiseImage(color, albedo, normal): the     Renderer.cs:686-700
 *   / pt_read_features denoiser's auxiliary images, here the true first-hit
 *   / pt_write_features albedo, shading normal and depth of one primary ray
 *   / pt_denoise_guided per pixel, and the à-trous filter guided by them
 *   pt_reset_buffer    Renderer.PBuffer = new Buffer(w,h)                  Renderer.cs:41
 *   pt_write_buffer    resuming IterativeRender from a saved PBuffer       Renderer.cs:702-765
 *   pt_read_tiles /    (new) a tile list's pixels, packed: progressive    SURVEY.md §8e
 *   pt_write_tiles     display of a rank's tiles, host-side gathers
 *   pt_intersect /     Scene.Intersect of a host's rays; the shadow query   Scene.cs:75-79, Sampler.cs:261-265
 *   pt_occluded
 *   pt_intersect_hits  Scene.Intersect of a host's rays with the Hit and its   Hit.cs:6-55, Scene.cs:75-79
 *                      Hit.Info: which shape, which triangle, where, the
 *                      normal, the side, the material and its colour
 *   pt_stats           Scene.rays (Interlocked counter, never printed)     Scene.cs:70-79
 *                      + the "time elapsed" stopwatch                      Renderer.cs:212-213,470
 *   pt_last_error      oidnGetDeviceError(device, out msg)                 OIDN.cs:85-86
 *   pt_destroy         oidnReleaseDevice                                   OIDN.cs:55-56
 *   pt_comm_*          (new) Buffer gather across GPUs over RCCL/xGMI      SURVEY.md §8e
 *                      (one process per GPU, or one process on all GPUs:  Renderer.cs:257-333 is one
 *                       pt_comm_init_all / pt_comm_gather_all)            process on all cores)
 *
 * Conventions: every function returns PT_OK (0) or a negative pt_status; the
 * detail string of the last failure on the calling thread is pt_last_error().
 * All structs are blittable POD (C# [StructLayout(LayoutKind.Sequential)]).
 * Geometry is float (the reference stores Vector as System.Numerics.Vector3,
 * Vector.cs:201), material/colour/camera scalars are double (Colour.cs:10-12,
 * Camera.cs:12-14).  Host arrays are caller-owned and are copied during the call.
 * A context is used by one host thread at a time; contexts are independent.
 */
#ifndef PTSHARP_HIP_H
#define PTSHARP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 10

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = -1,
    PT_ERR_HIP = -2,          /* a HIP runtime call failed (detail in pt_last_error) */
    PT_ERR_NO_SCENE = -3,     /* pt_render_pass before pt_upload_scene */
    PT_ERR_UNSUPPORTED = -4,  /* a shape/material feature the GPU path does not cover */
    PT_ERR_OUT_OF_MEMORY = -5,
    PT_ERR_RCCL = -6,
    PT_ERR_NO_DEVICE = -7
} pt_status;

/* Shape kinds in Scene.Shapes order (Scene.cs:19,29-38). */
typedef enum pt_shape_kind {
    PT_SHAPE_SPHERE = 0,    /* Sphere.cs   */
    PT_SHAPE_CUBE = 1,      /* Cube.cs     */
    PT_SHAPE_PLANE = 2,     /* Plane.cs    */
    PT_SHAPE_TRIANGLE = 3,  /* Triangle.cs, added directly to the scene (a boxed struct) */
    PT_SHAPE_MESH = 4,      /* Mesh.cs, a range of triangles with its own tree */
    PT_SHAPE_SDF = 5,       /* SDF.cs SDFShape (sphere-traced signed distance tree) */
    PT_SHAPE_VOLUME = 6,    /* Volume.cs (voxel grid, iso-window marching) */
    PT_SHAPE_TRANSFORMED = 7 /* TransformedShape.cs (instancing of one inner shape) */
} pt_shape_kind;

/* ---- §8f row 4: SDF.cs, Volume.cs, TransformedShape.cs ----------------------
 * SDF nodes form a tree (children listed in pt_scene_desc.sdf_children).  Vector-
 * valued parameters are the reference's fp32 Vector fields widened to double. */
typedef enum pt_sdf_op {
    PT_SDF_SPHERE = 0,        /* SphereSDF       params: Radius, Exponent                 SDF.cs:115-140 */
    PT_SDF_CUBE = 1,          /* CubeSDF         params: Size.xyz                          SDF.cs:142-195 */
    PT_SDF_CYLINDER = 2,      /* CylinderSDF     params: Radius, Height                    SDF.cs:197-252 */
    PT_SDF_CAPSULE = 3,       /* CapsuleSDF      params: A.xyz, B.xyz, Radius, Exponent    SDF.cs:254-285 */
    PT_SDF_TORUS = 4,         /* TorusSDF        params: MajorRadius, MinRadius, MajorExponent, MinorExponent  SDF.cs:287-319 */
    PT_SDF_TRANSFORM = 5,     /* TransformSDF    matrix, inverse; 1 child                  SDF.cs:321-353 */
    PT_SDF_SCALE = 6,         /* ScaleSDF        params: Factor; 1 child                   SDF.cs:355-382 */
    PT_SDF_UNION = 7,         /* UnionSDF        n children                                SDF.cs:384-435 */
    PT_SDF_DIFFERENCE = 8,    /* DifferenceSDF   n >= 1 children                           SDF.cs:437-477 */
    PT_SDF_INTERSECTION = 9,  /* IntersectionSDF n children                                SDF.cs:479-531 */
    PT_SDF_REPEAT = 10        /* RepeatSDF       params: Step.xyz; 1 child                 SDF.cs:533-559 */
} pt_sdf_op;

typedef struct pt_sdf_node {
    int32_t op;               /* pt_sdf_op */
    int32_t num_children;
    int32_t first_child;      /* children: sdf_children[first_child .. first_child + num_children) */
    int32_t _pad;
    double params[8];
    double matrix[16];        /* PT_SDF_TRANSFORM: Matrix M11..M44, row-major */
    double inverse[16];       /* and the Inverse TransformSDF stores */
} pt_sdf_node;

typedef struct pt_sdf_shape {  /* SDFShape.NewSDFShape(sdf, material), SDF.cs:12-113 */
    int32_t root;             /* node index */
    int32_t material;
} pt_sdf_shape;

typedef struct pt_volume_window {  /* Volume.VolumeWindow, Volume.cs:8-19 */
    double lo, hi;
    int32_t material;
    int32_t _pad;
} pt_volume_window;

typedef struct pt_volume {    /* Volume fields W, H, D, ZScale, Data, Windows, Box (Volume.cs:21-38) */
    int32_t w, h, d;
    int32_t num_windows;
    double zscale;
    const double* data;       /* [d][h][w] */
    const pt_volume_window* windows;
    float box_min[3];
    float box_max[3];
} pt_volume;

typedef struct pt_transformed_shape {  /* TransformedShape(Shape, Matrix, Inverse), TransformedShape.cs:9-24 */
    int32_t shape_kind;       /* inner IShape: SPHERE, CUBE, PLANE, SDF, VOLUME or MESH (an instanced mesh) */
    int32_t shape_index;      /* index into that kind's arrays */
    double matrix[16];
    double inverse[16];
} pt_transformed_shape;

/* ColorTexture (Texture.cs:96-252): Width x Height Colour texels, row-major, as the
 * C# object holds them (Data[y * Width + x], already through Pow(2.2) and any
 * ITexture.Pow / MulScalar the scene applied).  Width and Height must be >= 2
 * (BilinearSample reads texel x0 + 1 and y0 + 1, Texture.cs:198-206). */
typedef struct pt_texture {
    int32_t width;
    int32_t height;
    const double* data;   /* [height][width][3] */
} pt_texture;

/* Material (Material.cs:8-62).  Texture slots are 1-based references into
 * pt_scene_desc.textures: 0 = null (no map), k = textures[k - 1], so a zeroed
 * pt_material is a valid untextured material. */
typedef struct pt_material {
    double color[3];      /* Colour Color            */
    double emittance;     /* Emittance               */
    double index;         /* Index (IOR)             */
    double gloss;         /* Gloss (radians)         */
    double tint;          /* Tint                    */
    double reflectivity;  /* Reflectivity (<0: Fresnel) */
    int32_t transparent;  /* Transparent             */
    int32_t texture;          /* Texture       → Color (Material.MaterialAt, Material.cs:124-138)  */
    int32_t normal_texture;   /* NormalTexture → Triangle.NormalAt normal map (Triangle.cs:147-168) */
    int32_t bump_texture;     /* BumpTexture   → Triangle.NormalAt bump (Triangle.cs:170-184)       */
    int32_t gloss_texture;    /* GlossTexture  → Gloss = mean of the sampled colour               */
    int32_t _pad;
    double bump_multiplier;   /* BumpMultiplier */
} pt_material;

/* Flattened Scene.  Triangle arrays hold every triangle: directly-added ones
 * (shape_kind TRIANGLE, shape_index = triangle index) and mesh triangles
 * (mesh_first/mesh_count ranges).  Per-element arrays are [n][3] row-major. */
typedef struct pt_scene_desc {
    int32_t num_materials;
    const pt_material* materials;

    int32_t num_shapes;
    const int32_t* shape_kind;    /* pt_shape_kind, Scene.Shapes order */
    const int32_t* shape_index;   /* index into the per-kind arrays    */

    int32_t num_spheres;
    const float* sphere_center;   /* [n][3]  Sphere.Center (Vector) */
    const double* sphere_radius;  /* [n]     Sphere.Radius (double) */
    const int32_t* sphere_material;

    int32_t num_cubes;
    const float* cube_min;        /* [n][3] */
    const float* cube_max;        /* [n][3] */
    const int32_t* cube_material;

    int32_t num_planes;
    const float* plane_point;     /* [n][3] */
    const float* plane_normal;    /* [n][3], already normalised as Plane.NewPlane does */
    const int32_t* plane_material;

    int32_t num_triangles;
    const float* tri_v1;          /* [n][3] V1,V2,V3 */
    const float* tri_v2;
    const float* tri_v3;
    const float* tri_n1;          /* [n][3] N1,N2,N3 (after FixNormals / SmoothNormals) */
    const float* tri_n2;
    const float* tri_n3;
    const int32_t* tri_material;

    int32_t num_meshes;
    const int32_t* mesh_first;    /* first triangle of each mesh */
    const int32_t* mesh_count;

    double env_color[3];          /* Scene.Color (Scene.cs:25), returned on a miss */

    /* textures (§8f row 3); all optional */
    int32_t num_textures;
    const pt_texture* textures;
    const float* tri_t1;          /* [n][3] Triangle.T1..T3 texture coordinates; NULL = all zero */
    const float* tri_t2;
    const float* tri_t3;
    int32_t env_texture;          /* Scene.Texture (1-based, 0 = null): sampleEnvironment, Sampler.cs:177-189 */
    int32_t _pad;
    double env_texture_angle;     /* Scene.TextureAngle */

    /* SDF shapes, volumes, transformed shapes (§8f row 4); all optional */
    int32_t num_sdf_nodes;
    const pt_sdf_node* sdf_nodes;
    const int32_t* sdf_children;
    int32_t num_sdf_shapes;
    const pt_sdf_shape* sdf_shapes;
    int32_t num_volumes;
    const pt_volume* volumes;
    int32_t num_transformed;
    const pt_transformed_shape* transformed;
} pt_scene_desc;

/* Camera struct fields (Camera.cs:11-14) as produced by Camera.LookAt/SetFocus. */
typedef struct pt_camera {
    float p[3], u[3], v[3], w[3];
    double m;
    double focal_distance;
    double aperture_radius;
} pt_camera;

typedef enum pt_light_mode { PT_LIGHT_RANDOM = 0, PT_LIGHT_ALL = 1 } pt_light_mode;        /* LightMode.cs */
typedef enum pt_specular_mode { PT_SPEC_NAIVE = 0, PT_SPEC_FIRST = 1, PT_SPEC_ALL = 2 } pt_specular_mode; /* SpecularMode.cs */

/* DefaultSampler parameters (Sampler.cs:13-18).  FirstHitSamples/MaxBounces/
 * DirectLighting/SoftShadows are private in C#, so the drop-in passes them explicitly. */
typedef struct pt_sampler {
    int32_t first_hit_samples;
    int32_t max_bounces;
    int32_t direct_lighting;
    int32_t soft_shadows;
    int32_t light_mode;      /* pt_light_mode    */
    int32_t specular_mode;   /* pt_specular_mode */
} pt_sampler;

/* One render pass (one RenderParallel call).  Random.Shared is replaced by a
 * counter-based stream keyed (seed, pass_index, pixel, sample, path node, dim). */
typedef struct pt_pass_params {
    int32_t spp;             /* Renderer.SamplesPerPixel                         */
    int32_t stratified;      /* Renderer.StratifiedSampling (Renderer.cs:231-253) */
    uint64_t seed;
    uint32_t pass_index;     /* IterativeRender iteration i (Renderer.cs:709)    */
    int32_t num_tiles;       /* 0 = whole image; else render only these 32x32 tiles */
    const int32_t* tiles;    /* tile id = ty * ceil(W/32) + tx                   */
    int32_t engine;          /* pt_engine                                        */
    int32_t flags;           /* PT_PASS_KERNEL_TIMING: per-kernel hipEvent timing; PT_PASS_SERIAL */
    int32_t adaptive_samples;/* Renderer.AdaptiveSamples (Renderer.cs:340-410): per-sample AddSample x N */
    int32_t firefly_samples; /* Renderer.FireflySamples (Renderer.cs:412-470, FireflyThreshold = 1) */
    int32_t passes;          /* 0 or 1: one pass.  K > 1: K consecutive IterativeRender passes
                              * (pass_index .. pass_index + K - 1) in one call, the Buffer as after K
                              * separate calls, bit for bit.  Plain RenderParallel passes on the
                              * wavefront engine run as one batch: every pass' samples in one launch
                              * sequence, each pass' Welford update applied per pixel in order (a
                              * small tile share fills the GPU like a whole frame); other passes run
                              * one by one.  pt_stats then covers the K passes. */
} pt_pass_params;

#define PT_PASS_KERNEL_TIMING 1
/* Renderer.Render semantics (Renderer.cs:80-198, taken by IterativeRender when NumCPU == 1,
 * Renderer.cs:712-719) instead of RenderParallel's: the main samples are the same; then per
 * pixel AdaptiveSamples individual samples when StandardDeviation().MaxComponent() >= 1
 * (AdaptiveSamples * (int)v, AdaptiveThreshold = AdaptiveExponent = 1, :153-175), then
 * FireflySamples individual samples when it exceeds 1 (:177-191; no IsFirefly stop, jitter
 * (x + NextDouble()) * (1.0f / w)). */
#define PT_PASS_SERIAL 2

/* Kernel classes reported by pt_stats.kernel_ms / kernel_launches. */
typedef enum pt_kernel_class {
    PT_K_CAMERA = 0, PT_K_TRACE = 1, PT_K_SHADE = 2, PT_K_SHADOW = 3, PT_K_FINALIZE = 4, PT_K_MEGAKERNEL = 5,
    PT_K_ACCUM = 6,            /* k_wf_nee_accum: the visible shadow rays' light terms into the pixel sums */
    PT_K_COUNT = 7
} pt_kernel_class;
#define PT_K_SLOTS 8           /* length of pt_stats.kernel_ms / kernel_launches */
/* Slot 7 is not a pass' kernel class: the last pt_read_image's kernels (device time between two
 * hipEvents, always taken, and their launches).  Like the other slots it is cleared by the next pass. */
#define PT_K_IMAGE 7

/* Both engines compute identical per-ray arithmetic; they differ in scheduling. */
typedef enum pt_engine {
    PT_ENGINE_AUTO = 0,        /* wavefront, megakernel when the queues cannot hold a useful chunk */
    PT_ENGINE_MEGAKERNEL = 1,  /* one lane per pixel runs the whole sampler recursion */
    PT_ENGINE_WAVEFRONT = 2    /* depth-by-depth ray queues in HBM (trace / shade / shadow kernels) */
} pt_engine;

typedef struct pt_device_opts {
    int32_t device;          /* HIP device ordinal */
    int32_t width;
    int32_t height;
} pt_device_opts;

typedef struct pt_stats {
    uint64_t rays;           /* Scene.Intersect calls, last pass (Scene.cs:77) */
    uint64_t rays_total;     /* since pt_create / pt_reset_buffer             */
    double last_pass_ms;     /* device time of the last pass (hipEvent)       */
    double total_ms;
    uint64_t bvh_nodes;      /* acceleration structure size                   */
    uint64_t bvh_bytes;
    double build_ms;         /* host BVH build time of the last upload        */
    uint64_t passes;
    uint64_t shadow_rays;    /* of `rays`: shadow-visibility queries (sampleLight)     */
    double kernel_ms[PT_K_SLOTS];     /* last pass, device time per pt_kernel_class (flag PT_PASS_KERNEL_TIMING) */
    uint32_t kernel_launches[PT_K_SLOTS];
    uint64_t traversal_bytes; /* of bvh_bytes: BVH nodes + leaf chunks, what the traversal kernels read */
    uint64_t tail_handoffs;   /* last pass (ABI 9): stack entries the shadow refill kernel's idle lanes took from
                               * busy lanes' rays in its tail (k_wf_shadow_lanes helpers; wavefront engine) */
} pt_stats;

int pt_get_version(void);
int pt_device_count(int32_t* out_count);
int pt_create(const pt_device_opts* opts, void** out_ctx);
int pt_upload_scene(void* ctx, const pt_scene_desc* scene);
int pt_render_pass(void* ctx, const pt_camera* camera, const pt_sampler* sampler,
                   const pt_pass_params* pass);
int pt_synchronize(void* ctx);
int pt_reset_buffer(void* ctx);
/* Welford state of every pixel, row-major: M,V [H*W][3] (Colour, double), N [H*W]. */
int pt_read_buffer(void* ctx, double* out_m, double* out_v, int32_t* out_n);
/* Replace the Welford state (same layout; NULL leaves that array as it is): resume an
 * IterativeRender from a saved Buffer (Renderer.cs:702-765 keeps accumulating into
 * Renderer.PBuffer pass after pass; a checkpoint is that Buffer). */
int pt_write_buffer(void* ctx, const double* m, const double* v, const int32_t* n);

/* Buffer.Image(channel) (Buffer.cs:134-282) resolved on the device: the context's Buffer as it
 * stands (a tile-sharded context: its own tiles, zero pixels elsewhere; the root after a gather:
 * the whole frame) as 8-bit colour, row-major, into the caller's `out`: [H][W][3] (PT_IMAGE_RGB8)
 * or [H][W][4] with A = 255 (PT_IMAGE_RGBA8, the SKColor(r, g, b, 255) of Buffer.cs:160).  Every
 * channel ends in (byte)Math.Clamp(c·255, 0, 255) with a NaN mapped to 0; the arithmetic is fp64 in
 * the reference's order (ptsharp_amd/csrc/pt_image.h).  Runs on the context's stream after every
 * pass issued before it and synchronises before returning; it changes neither the Buffer nor any
 * pass state, and needs no scene.  A NULL ctx or out, or a channel or format outside the enums:
 * PT_ERR_INVALID_ARG, nothing launched. */
typedef enum pt_channel { PT_CHANNEL_COLOR = 0, PT_CHANNEL_VARIANCE = 1, PT_CHANNEL_STDDEV = 2,
                          PT_CHANNEL_SAMPLES = 3, PT_CHANNEL_ALBEDO = 4, PT_CHANNEL_NORMAL = 5 } pt_channel;  /* Buffer.cs:8-16 */
typedef enum pt_image_format { PT_IMAGE_RGB8 = 0, PT_IMAGE_RGBA8 = 1 } pt_image_format;
int pt_read_image(void* ctx, int32_t channel, int32_t format, uint8_t* out);

/* Renderer.Denoise (Renderer.cs:731-761), served natively: an edge-avoiding à-trous wavelet filter
 * (Dammertz et al. 2010) whose colour weight is scaled by each pixel's own variance of the mean,
 * V / ((N-1)·N) from the Welford state (a spatial 5x5 estimate while N < 2), all in fp64
 * (ptsharp_amd/csrc/pt_denoise.h).  Intel OIDN, the reference's denoiser, is not used. */
typedef struct pt_denoise_params {
    int32_t iterations;      /* 1..8 levels, step 2^j at level j */
    int32_t reserved;        /* 0 */
    double  sigma_colour;    /* > 0, finite */
} pt_denoise_params;

/* Filters the Buffer as it stands into a context-owned result (allocated on first use, freed by
 * pt_destroy; PT_ERR_OUT_OF_MEMORY if it cannot be had).  Changes neither the Buffer nor any pass
 * state; needs no scene.  params NULL = defaults (5 iterations, sigma_colour 4.0).  out_kernel_ms
 * (may be NULL): device time of the call's kernels between two hipEvents.  Runs on the context's
 * stream after every pass issued before it and synchronises before returning.  A tile-sharded
 * context filters what it holds (its foreign pixels have N = 0 and are invalid: never a tap, passed
 * through as centres); the root after a gather filters the whole frame.  A NULL ctx, iterations
 * outside 1..8, a sigma_colour that is not finite and positive, or reserved != 0:
 * PT_ERR_INVALID_ARG, nothing launched. */
int pt_denoise(void* ctx, const pt_denoise_params* params, double* out_kernel_ms);

/* The last pt_denoise's result, row-major, into the caller's `out`.  The result is a snapshot: later
 * passes do not change it.  The 8-bit formats encode the denoised colour exactly as pt_read_image
 * encodes the Color channel.  pt_denoise_guided leaves its result in the same place.  Before any
 * pt_denoise or pt_denoise_guided on the context, a NULL ctx or out, or a format outside the enum:
 * PT_ERR_INVALID_ARG. */
typedef enum pt_denoised_format { PT_DENOISED_RGB8 = 0, PT_DENOISED_RGBA8 = 1,
                                  PT_DENOISED_COLOUR_F64 = 2,    /* [H][W][3] double, linear */
                                  PT_DENOISED_VARIANCE_F64 = 3   /* [H][W][3] double, the propagated s2 */
} pt_denoised_format;
int pt_read_denoised(void* ctx, int32_t format, void* out);

/* First-hit features of the whole frame, whatever tile list the context renders: one ray per pixel
 * (x, y), Camera.CastRay(x, y, W, H, 0.5, 0.5) with the lens ignored (aperture_radius is treated as
 * 0, so no random number is drawn and the pass is deterministic), its nearest hit by Scene.Intersect
 * and Hit.Info there: the shading normal after the flip (normal and bump maps included), the material
 * id and the Material.MaterialAt colour.  On a miss the kind is -1, the depth Hit.INF (1e9), the
 * normal (0,0,0), the material -1 and the albedo sampleEnvironment(direction).  The features are
 * context-owned (allocated on first use, freed by pt_destroy; PT_ERR_OUT_OF_MEMORY if they cannot be
 * had).  Runs on the context's stream after every pass issued before it and synchronises before
 * returning; changes neither the Buffer nor any pass state or counter.  out_kernel_ms may be NULL.
 * Needs an uploaded scene (PT_ERR_NO_SCENE); a NULL ctx or camera: PT_ERR_INVALID_ARG. */
int pt_render_features(void* ctx, const pt_camera* camera, double* out_kernel_ms);

/* One feature of the last pt_render_features or pt_write_features, row-major, into `out`.  Before
 * either on the context, a NULL ctx or out, or a feature outside the enum: PT_ERR_INVALID_ARG. */
typedef enum pt_feature { PT_FEATURE_ALBEDO_F64 = 0,     /* [H][W][3] double */
                          PT_FEATURE_NORMAL_F32 = 1,     /* [H][W][3] float */
                          PT_FEATURE_DEPTH_F64 = 2,      /* [H][W] double, the ray's t; 1e9 on a miss */
                          PT_FEATURE_KIND_I32 = 3,       /* [H][W] int32, the pt_shape_kind hit as pt_intersect reports it, or -1 */
                          PT_FEATURE_MATERIAL_I32 = 4    /* [H][W] int32, the material id, or -1 */
} pt_feature;
int pt_read_features(void* ctx, int32_t feature, void* out);

/* Installs a host's own features (its AOVs), as pt_write_buffer installs a Buffer: all four arrays
 * are required (layouts as pt_read_features; a pixel is a hit where kind >= 0), the material becomes
 * -1 everywhere, and the filter's guide records are rebuilt on the device.  Needs no scene. */
int pt_write_features(void* ctx, const double* albedo, const float* normal, const double* depth, const int32_t* kind);

/* pt_denoise guided by the context's features.  Prepare, the variance blur, the levels, the validity
 * rules and the variance propagation are pt_denoise's; only a tap's weight changes.  With the guide
 * values (fp32 copies of normal, depth and albedo, and the hit flag) widened to fp64, a tap whose hit
 * flag differs from the centre's is skipped like an invalid tap, and for the others
 *   w(q) = h(dx,dy) · exp(−d),  d = d_colour                                   (pt_denoise's term)
 *        + Σ_k (a_q,k − a_p,k)² / sigma_albedo²                                 if sigma_albedo > 0
 *        + Σ_k (n_q,k − n_p,k)² / sigma_normal²                                 if p is a hit and sigma_normal > 0
 *        + (z_q − z_p)² / (sigma_depth · z_p)²                                  if p is a hit and sigma_depth > 0
 * (ptsharp_amd/csrc/pt_denoise.h). */
typedef struct pt_denoise_guided_params {
    int32_t iterations;      /* 1..8 */
    int32_t reserved;        /* 0 */
    double  sigma_colour;    /* > 0, finite */
    double  sigma_normal;    /* >= 0, finite; 0 = term off */
    double  sigma_albedo;    /* likewise */
    double  sigma_depth;     /* likewise; relative to the centre's depth */
} pt_denoise_guided_params;

/* The result goes where pt_denoise's goes: pt_read_denoised returns the last pt_denoise or
 * pt_denoise_guided.  params NULL = defaults (5 iterations, sigma_colour 4.0, sigma_normal 0.3,
 * sigma_albedo 0.3, sigma_depth 0.1).  Stream order, out_kernel_ms and the Buffer as for pt_denoise.
 * No features on the context (no pt_render_features or pt_write_features before), a NULL ctx, or a field out of range:
 * PT_ERR_INVALID_ARG, nothing launched, out_kernel_ms untouched. */
int pt_denoise_guided(void* ctx, const pt_denoise_guided_params* params, double* out_kernel_ms);

/* The Buffer pixels of `num_tiles` 32x32 tiles, packed: m, v [num_tiles][32][32][3], n
 * [num_tiles][32][32], row-major inside a tile (entry (t, r, c) = pixel (32·(tiles[t] mod
 * ceil(W/32)) + c, 32·(tiles[t] div ceil(W/32)) + r)).  Pixels outside the image read as 0
 * and are ignored on write.  The same packing carries pt_comm_gather's tiles; a host that
 * moves Buffers over its own transport (gloo, MPI, sockets) gathers with these two calls. */
int pt_read_tiles(void* ctx, const int32_t* tiles, int32_t num_tiles, double* out_m, double* out_v, int32_t* out_n);
int pt_write_tiles(void* ctx, const int32_t* tiles, int32_t num_tiles, const double* m, const double* v,
                   const int32_t* n);
int pt_stats_get(void* ctx, pt_stats* out_stats);
const char* pt_last_error(void);
void pt_destroy(void* ctx);

/* ---- Mesh ingest (host only; no device needed).  OBJ.Load (OBJ.cs:11-165) with its
 * quirks: lower-cased lines split on ' ', the dummy normal 0, "v//n"
 * read as a texture index, fan triangulation, Triangle.FixNormals.  Arrays are [n][3]
 * float, allocated by the library; release them with pt_mesh_free. */
typedef struct pt_mesh_data {
    int32_t num_triangles;
    float *v1, *v2, *v3;   /* Triangle.V1..V3 */
    float *n1, *n2, *n3;   /* Triangle.N1..N3 (after FixNormals) */
    float *t1, *t2, *t3;   /* Triangle.T1..T3 (u, v, 0) */
} pt_mesh_data;
int pt_obj_load(const char* path, pt_mesh_data* out);
void pt_mesh_free(pt_mesh_data* mesh);
const char* pt_obj_last_error(void);
/* Mesh.SmoothNormals (Mesh.cs:191-229), in place on n1..n3. */
int pt_mesh_smooth_normals(int32_t n, const float* v1, const float* v2, const float* v3, float* n1, float* n2,
                           float* n3);

/* Multi-GPU: one context per GPU.  Each context renders its tile list
 * (pt_pass_params.tiles; the ranks' lists must be disjoint), and pt_comm_gather assembles
 * them on rank `root`: every other rank packs the {M, V, N} of its last pass' tiles and sends
 * them with the tile ids (RCCL send/recv over xGMI, after an all-gather of the tile counts);
 * root writes them into its Buffer.  For disjoint tiles that is the sum of the ranks'
 * Buffers, at 1/N of a full frame's bytes per rank.  Two ways to form the communicator:
 *   - one process per GPU: rank 0 makes the id (pt_comm_unique_id), ships it to the other
 *     processes, and every rank calls pt_comm_init (it blocks until all ranks joined);
 *   - one process driving G GPUs (the .NET host): G contexts on G devices, joined by ONE
 *     call pt_comm_init_all from any thread, gathered by pt_comm_gather_all.  Render the G
 *     contexts from G host threads at once (one thread per context): a pass with
 *     firefly_samples > 0 all-reduces the firefly snapshot across the group.
 * After a gather, root's pt_read_buffer returns the whole frame; root's next pass first
 * clears the pixels outside its own tiles again, so gathers can repeat every pass (so does any
 * rank's next tile-subset pass after pt_write_buffer or pt_write_tiles put other ranks' pixels in
 * its Buffer, e.g. every rank resuming from the whole checkpoint).  Root refuses a gather whose
 * tile ids repeat (two ranks rendered one tile) before it writes anything. */
int pt_comm_unique_id(uint8_t out_id[128]);
int pt_comm_init(void* ctx, int32_t nranks, int32_t rank, const uint8_t id[128]);
int pt_comm_gather(void* ctx, int32_t root);
int pt_comm_destroy(void* ctx);
int pt_comm_init_all(void* const* ctxs, int32_t n);            /* ncclCommInitAll over the contexts' devices */
int pt_comm_gather_all(void* const* ctxs, int32_t n, int32_t root);   /* the group's gathers, issued together */
/* The gather's host-side arithmetic, exported so a host can check its tile assignment before any
 * RCCL call (pure functions: no device, no context).  pt_gather_layout: where rank p's packed
 * tiles land in root's receive buffers (tile offset; -1 for root and for ranks with no tiles),
 * and the tiles root receives; PT_ERR_INVALID_ARG if a count is out of range or the counts sum
 * past image_tiles (overlapping lists).  pt_tile_lists_check: every id in [0, image_tiles), none
 * twice.  (Renderer.cs:257-333 deals disjoint sub-tiles to tasks; these keep the ranks disjoint.) */
int pt_gather_layout(int32_t nranks, int32_t root, const int32_t* counts, int32_t image_tiles,
                     int64_t* out_offsets, int64_t* out_total);
int pt_tile_lists_check(const int32_t* ids, int64_t n, int32_t image_tiles);

/* Ray queries on the uploaded scene, one lane per ray (the megakernel's traversal).  Rays are
 * [n][3] float origins and directions (Ray.Origin / Ray.Direction, Vector = Vector3).
 *   pt_intersect  Scene.Intersect (Scene.cs:75-79 → Tree.Intersect, Tree.cs:31-42): out_t[i] the
 *                 nearest hit's T (Hit.T, 1e9 = Hit.INF on a miss, Hit.cs:6), out_kind[i] its
 *                 pt_shape_kind (a mesh triangle is PT_SHAPE_TRIANGLE) or -1.
 *   pt_occluded   the shadow query after the light's own t (Sampler.cs:261-265 as the wavefront engine
 *                 answers it): out_blocked[i] = 1 if some shape is hit strictly nearer
 *                 than t_max[i].  Its walk of the analytic BVH does not cull boxes against t_max: a hit
 *                 distance carries the rounding of the shape's fp32 intersection and can fall short of
 *                 the entry distance of the shape's own box; a render's shadow rays cull.
 * flags choose how a ray's Volume (Volume.Intersect, Volume.cs:168-197) is marched; every choice
 * returns the same bits, which is what the flags are for: 0 as in a render (a wave's lanes march
 * together unless fewer than 8 are active), PT_MARCH_LANE every lane its own march, PT_MARCH_WAVE
 * always together. */
#define PT_MARCH_LANE 1
#define PT_MARCH_WAVE 2
int pt_intersect(void* ctx, int64_t n, const float* origins, const float* dirs, int32_t flags, double* out_t,
                 int32_t* out_kind);
int pt_occluded(void* ctx, int64_t n, const float* origins, const float* dirs, const double* t_max, int32_t flags,
                int32_t* out_blocked);

/* Ray queries that say what was hit and where: pt_intersect's query with the identity of the hit in the
 * host's own numbering and, when wanted, Hit.Info (Hit.cs:26-55) there.  Rays and flags as for pt_intersect; n in
 * [0, 2^30].  Every pointer of pt_hit_arrays may be NULL: that output is not wanted.  Asking for none of position ..
 * gloss runs a kernel that does not evaluate Hit.Info: pt_intersect's trace plus a few table lookups per ray.
 * A miss: t = 1e9; kind, index, prim, shape and material -1; position and normal (0,0,0); inside and gloss 0; albedo
 * the environment (sampleEnvironment(direction), as pt_render_features writes it).
 * shape: for an analytic shape or a plane the slot whose (shape_kind, shape_index) names it; for a triangle of the world
 * BVH the slot of the PT_SHAPE_TRIANGLE that names it, else of the mesh it belongs to (the last mesh_first / mesh_count
 * range that contains it, as for PT_NORMALS_SMOOTH and pt_pose_meshes; should that mesh be in no slot, the first slot of
 * a mesh that contains it); a hit through an instance reports the PT_SHAPE_TRANSFORMED slot.  Where several slots name
 * one shape, the first.
 * index, prim and shape name the scene as uploaded and stay what they were after pt_update_*, pt_pose_meshes and
 * pt_rebuild_meshes (the source numbering never changes); t, position and normal follow the moved geometry.  Where two
 * primitives are hit at exactly the same t, the one reported is the traversal's: any of them.
 * Rays and answers are staged in chunks of at most 2^22 rays (the environment's PT_QUERY_CHUNK, read at each call and
 * clamped to [64, 2^22], lowers it; the answers do not depend on it).  Runs on the context's stream after every pass
 * issued before it and synchronises before returning; changes neither the Buffer, the pass state, the counters nor the
 * feature buffers.  The identity tables (a few bytes per triangle and shape) are uploaded by the scene's first query and
 * kept until the next upload.
 * Errors (nothing launched, no output written): a NULL ctx or out, NULL origins or dirs with n > 0, reserved != 0, n
 * out of range, bad flags: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the staging or the tables not allocated:
 * PT_ERR_OUT_OF_MEMORY.  n = 0, or every pointer NULL: PT_OK, nothing launched.
 * pt_query_kernel_ms: the device time of the last pt_intersect_hits' kernels on the context (hipEvents around each
 * chunk's launch, summed); 0 when that call launched nothing. */
typedef struct pt_hit_arrays {      /* every pointer may be NULL: that output is not wanted */
    int32_t reserved[2];            /* 0 */
    double*  t;         /* [n]     Hit.T; 1e9 (Hit.INF) on a miss: pt_intersect's, bit for bit */
    int32_t* kind;      /* [n]     pt_shape_kind as pt_intersect reports it, or -1 */
    int32_t* index;     /* [n]     index into that kind's pt_scene_desc arrays: sphere, cube, plane, sdf_shapes, volumes,
                                   transformed; for PT_SHAPE_TRIANGLE the source triangle (tri_v1 row); -1 on a miss */
    int32_t* prim;      /* [n]     the source triangle whose surface was hit: == index for PT_SHAPE_TRIANGLE, the mesh's
                                   triangle for a pt_transformed_shape over PT_SHAPE_MESH, else -1 */
    int32_t* shape;     /* [n]     slot in Scene.Shapes order (pt_scene_desc.shape_kind / shape_index) of the top-level
                                   shape hit; -1 on a miss */
    float*   position;  /* [n][3]  Hit.Info's Position (ray.Position(T)) */
    float*   normal;    /* [n][3]  Hit.Info's Normal after the flip, normal and bump maps applied */
    int32_t* inside;    /* [n]     Hit.Info's Inside */
    int32_t* material;  /* [n]     material id, as pt_read_features' PT_FEATURE_MATERIAL_I32 */
    double*  albedo;    /* [n][3]  Material.MaterialAt colour; on a miss sampleEnvironment(direction) */
    double*  gloss;     /* [n]     MaterialAt gloss (gloss texture applied) */
} pt_hit_arrays;
int pt_intersect_hits(void* ctx, int64_t n, const float* origins, const float* dirs, int32_t flags,
                      const pt_hit_arrays* out);
int pt_query_kernel_ms(void* ctx, double* out_ms);

/* The triangle BVH is built once per process for identical geometry: N contexts that upload the same
 * scene (one process driving N GPUs) share one host build (Scene.Compile once, Scene.cs:48-68) and upload
 * its bytes; a context that uploads while another builds waits for that build.  Host only (no device):
 * out[0] a 64-bit digest of the BVH bytes a context of this scene receives (node lines, leaf chunks,
 * triangle order), out[1] their size in bytes, out[2] / out[3] the builds made / builds reused so far. */
int pt_scene_bvh_digest(const pt_scene_desc* scene, uint64_t out[4]);

/* New vertex positions (and optionally normals) for every triangle of the uploaded scene, in
 * pt_scene_desc order; topology, materials, texture coordinates and every other shape stay.  The
 * triangle BVH is refitted on the device: afterwards every ray query, feature pass and
 * render pass sees the scene a fresh pt_upload_scene of the same pt_scene_desc with these arrays would
 * see, up to the exact-t tie order of DESIGN.md §5.  Runs on the context's stream after every pass issued
 * before it and synchronises before returning; out_kernel_ms (may be NULL) is the device time of its
 * kernels.  The Buffer, the pass state and the counters are unchanged.  Lights that are emissive
 * triangles added directly to the scene follow their triangle.
 * Errors (nothing launched, the scene untouched): a NULL ctx, v1, v2 or v3, normals partly NULL, or
 * num_triangles different from the uploaded scene's: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; a scene
 * with an instanced mesh (a pt_transformed_shape whose shape_kind is PT_SHAPE_MESH): PT_ERR_UNSUPPORTED.
 * A scene without triangles and num_triangles 0: PT_OK, nothing launched. */
int pt_update_triangles(void* ctx, int32_t num_triangles,
                        const float* v1, const float* v2, const float* v3,   /* [n][3], required */
                        const float* n1, const float* n2, const float* n3,   /* [n][3]; all three or all NULL = keep */
                        double* out_kernel_ms);
/* The context's triangle BVH as it stands on the device (tests and tools): counts[0..2] = nodes, leaf
 * chunks, triangle records; each non-NULL array receives 32 words per node / chunk / record;
 * out_box[6] = the root box the traversal tests first.  Any argument but ctx may be NULL. */
int pt_read_tri_bvh(void* ctx, int64_t counts[3], uint32_t* nodes, uint32_t* chunks, uint32_t* records, float out_box[6]);

/* pt_update_triangles with the normals derived on the device from the new positions: everything
 * pt_update_triangles does with v1..v3 and given normals happens here, the normals being computed, not given.
 *   PT_NORMALS_FACE    every corner of a triangle takes Triangle.Normal(), normalize(cross(V2 - V1, V3 - V1)) in
 *                      fp32, each operation rounded on its own (Triangle.FixNormals on zeroed normals).
 *   PT_NORMALS_SMOOTH  the face normals, then Mesh.SmoothNormals (Mesh.cs:191-229) on each mesh (a
 *                      mesh_first / mesh_count range of the uploaded pt_scene_desc) by itself: per distinct vertex
 *                      position of the mesh the fp32 sum of its corners' normals from (+0, +0, +0) in ascending
 *                      (triangle, corner 1-2-3) order, normalised; every corner at that position takes it.
 *                      Positions compare as Vector == (-0 and +0 are one position).  Meshes that share positions
 *                      do not share sums; a triangle outside every mesh keeps its face normal; a triangle inside
 *                      several ranges belongs to the last of them.  The result is pt_mesh_smooth_normals' on the
 *                      face normals, bit for bit (a NaN where that gives a NaN: a zero-area triangle poisons its
 *                      vertices; payloads may differ), and does not depend on the run.
 * Non-finite positions (the reference throws): the normals of corners at such a position, and of triangles that
 * have one, are unspecified; every other normal is as above, and no access leaves its array.
 * out_kernel_ms (may be NULL) covers every kernel of the call: the normals, the sort, the refit.
 * Errors (nothing launched, the scene untouched): those of pt_update_triangles, a mode outside pt_normals_mode:
 * PT_ERR_INVALID_ARG; PT_NORMALS_SMOOTH's workspace (about 60 B per triangle, kept until the next upload) not
 * allocated: PT_ERR_OUT_OF_MEMORY; PT_NORMALS_SMOOTH with 3 * num_triangles >= 2^31: PT_ERR_UNSUPPORTED. */
typedef enum pt_normals_mode { PT_NORMALS_FACE = 1, PT_NORMALS_SMOOTH = 2 } pt_normals_mode;
int pt_update_triangles_normals(void* ctx, int32_t num_triangles,
                                const float* v1, const float* v2, const float* v3,   /* [n][3], required */
                                int32_t mode, double* out_kernel_ms);
/* The normals the uploaded scene holds on the device now, [n][3] each in pt_scene_desc order (a triangle that is
 * in no shape of the scene has none: zeros).  Valid any time after an upload; synchronises and changes nothing.
 * A NULL ctx or output: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_read_tri_normals(void* ctx, float* n1, float* n2, float* n3);

/* New parameters for the spheres, cubes and transformed shapes of the uploaded scene: a
 * sphere's centre and radius, a cube's corners, the matrix of a pt_transformed_shape (an instanced mesh
 * included: the instance moves rigidly, its BLAS stays).  A group is given when its first pointer is non-NULL;
 * a given group's count must equal the uploaded scene's; arrays are in pt_scene_desc order and are copied during
 * the call.  The analytic BVH is refitted on the device with its topology kept: afterwards every ray query,
 * feature pass and render pass sees the scene a fresh pt_upload_scene of the same pt_scene_desc with these
 * arrays substituted would see, up to the exact-t tie order of DESIGN.md §5.  Records, ext records,
 * transforms, the boxes the routed split tests and the lights that are spheres, cubes or transformed shapes
 * follow.  The triangle BVH, BLASes, materials, textures, SDF programs, volumes, planes, the Buffer, the pass
 * state and the counters are untouched.  Runs on the context's stream after every pass issued before it and
 * synchronises before returning; out_kernel_ms (may be NULL) is the device time of its kernels.  It composes
 * with pt_update_triangles in either order.  Non-finite values: what they do to the boxes is unspecified; no
 * access leaves its array.
 * Errors (nothing launched, the scene untouched): a NULL ctx or u, reserved != 0, cube_min / cube_max or
 * xform_matrix / xform_inverse half given, sphere_radius without sphere_center, a given group's count
 * different from the scene's: PT_ERR_INVALID_ARG (the values themselves are checked as pt_upload_scene checks
 * them: not at all); no scene: PT_ERR_NO_SCENE; the workspace (kept until the next upload) not allocated:
 * PT_ERR_OUT_OF_MEMORY.  No group given, or a scene without analytic records: PT_OK, nothing launched. */
typedef struct pt_shape_update {
    int32_t num_spheres, num_cubes, num_transformed, reserved;   /* reserved = 0 */
    const float*  sphere_center;   /* [num_spheres][3]; NULL = spheres stay */
    const double* sphere_radius;   /* [num_spheres];    NULL = radii stay   */
    const float*  cube_min;        /* [num_cubes][3];   both or neither     */
    const float*  cube_max;
    const double* xform_matrix;    /* [num_transformed][16] row-major; both or neither */
    const double* xform_inverse;
} pt_shape_update;
int pt_update_shapes(void* ctx, const pt_shape_update* u, double* out_kernel_ms);
/* The context's analytic BVH as it stands on the device (tests and tools): counts[0..3] = BVH4 nodes, analytic
 * records, heavy records, lights; each non-NULL array receives 32 words per node, 12 words per record, 8 words
 * per heavy record, 4 doubles per light (centre x, y, z widened to double, then the radius).  Any argument but
 * ctx may be NULL.  Synchronises and changes nothing. */
int pt_read_shape_bvh(void* ctx, int64_t counts[4], uint32_t* nodes, uint32_t* recs, uint32_t* heavy, double* lights);

/* pt_update_triangles and pt_update_triangles_normals in one struct-based entry point that also serves a scene
 * with instanced meshes (those two still refuse such a scene).  New positions for every triangle of
 * the uploaded scene, in pt_scene_desc order, the triangles of instanced meshes included, whether or not the mesh
 * is also a top-level shape; the normals given (normals_mode 0, n1..n3 all set), kept (normals_mode 0, n1..n3 all
 * NULL) or derived (PT_NORMALS_FACE, PT_NORMALS_SMOOTH: as pt_update_triangles_normals derives them, an instanced
 * mesh being a mesh like any other).
 * A scene without an instanced mesh: everything on the device is, word for word, what those two calls leave.
 * A scene with instanced meshes: besides the world triangle BVH, every BLAS (the object-space BVH of an instanced
 * mesh) is refitted with its topology kept: its triangles' geometry rows, their normal rows when normals are given
 * or derived (the material word kept), every node's child boxes; then each mesh's unpadded Mesh.BoundingBox, the
 * inner box of every pt_transformed_shape over it; then, through pt_update_shapes' refit from the current sphere,
 * cube and matrix values, those shapes' world boxes, the analytic BVH, the boxes the routed split tests and the
 * lights made from such shapes.  Afterwards every ray query, feature pass and render pass sees the scene a fresh
 * pt_upload_scene of the same pt_scene_desc with these arrays and the current shape parameters would see, up to the
 * exact-t tie order of DESIGN.md §5.  Texture coordinates, materials, topology, the Buffer, the pass state and the
 * counters are untouched.  Runs on the context's stream after every pass issued before it and synchronises before
 * returning; out_kernel_ms (may be NULL) covers every kernel of the call.  It composes with pt_update_shapes in
 * either order.  Non-finite positions: boxes and normals are unspecified; no access leaves its array.
 * Errors (nothing launched, the scene untouched): a NULL ctx, u, v1, v2 or v3, reserved != 0, a normals_mode outside
 * {0, 1, 2}, normals partly NULL or given with normals_mode != 0, num_triangles different from the uploaded scene's:
 * PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; a workspace (kept until the next upload) not allocated:
 * PT_ERR_OUT_OF_MEMORY; PT_NORMALS_SMOOTH with 3 * num_triangles >= 2^31: PT_ERR_UNSUPPORTED. */
typedef struct pt_mesh_update {
    int32_t num_triangles;     /* must equal the uploaded scene's */
    int32_t normals_mode;      /* 0: n1..n3 given (all three) or kept (all NULL); PT_NORMALS_FACE; PT_NORMALS_SMOOTH */
    int32_t reserved[2];       /* 0 */
    const float *v1, *v2, *v3; /* [n][3], required, pt_scene_desc order */
    const float *n1, *n2, *n3; /* [n][3]; only with normals_mode 0 */
} pt_mesh_update;
int pt_update_meshes(void* ctx, const pt_mesh_update* u, double* out_kernel_ms);
/* The context's BLASes as they stand on the device (tests and tools): counts[0..2] = BLASes, BLAS nodes in total,
 * BLAS triangles in total; blas receives 4 int32 per BLAS (first node, nodes, first triangle, 0), nodes 32 words
 * per node (child references and leaf firsts are relative to the BLAS's first node / triangle), recs and shade 12
 * words per triangle position each, inner_boxes 6 floats per BLAS: the unpadded mesh box (min, max) the device holds
 * after a pt_update_meshes, the upload's before.  A triangle that is only instanced reads as zeros in
 * pt_read_tri_normals; its normals are in shade.  Any argument but ctx may be NULL.  Synchronises and changes
 * nothing.  A NULL ctx: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_read_blas(void* ctx, int64_t counts[3], int32_t* blas, uint32_t* nodes, uint32_t* recs, uint32_t* shade, float* inner_boxes);

/* Posing meshes by matrix on the device: Mesh.Transform (Mesh.cs:254-274) of every mesh of the
 * uploaded scene, top-level, instanced or both, from a rest pose kept on the device, so that a frame sends one 4x4
 * matrix per mesh and not every vertex.
 *
 * pt_set_rest_pose installs the rest pose: positions and normals of every triangle, pt_scene_desc order, copied to a
 * device buffer (72 B per triangle) kept until the next pt_upload_scene.  All six arrays are required.  It changes
 * nothing a ray sees.  Errors: a NULL ctx or array, num_triangles different from the uploaded scene's:
 * PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the buffer not allocated: PT_ERR_OUT_OF_MEMORY. */
int pt_set_rest_pose(void* ctx, int32_t num_triangles,
                     const float* v1, const float* v2, const float* v3,
                     const float* n1, const float* n2, const float* n3);
/* pt_pose_meshes poses the rest pose and refits.  A source triangle belongs to the last mesh_first / mesh_count range
 * of the uploaded pt_scene_desc that contains it (as for PT_NORMALS_SMOOTH), or to none (a loose triangle).  The
 * triangles of an unmasked mesh g get V' = Matrix.MulPosition(matrices[g], V_rest) and, with normals_mode 0,
 * N' = Matrix.MulDirection(matrices[g], N_rest): Matrix.cs:134-150 exactly, fp64 products summed left to right, one
 * conversion to fp32, then the fp32 Normalize (the fourth row of a matrix is not read).  Loose triangles and the
 * triangles of a masked mesh take their rest values bit for bit.  With PT_NORMALS_FACE or PT_NORMALS_SMOOTH the
 * normals of every triangle are derived from the posed positions as pt_update_meshes derives them; the mask then
 * governs positions only.  A pose is always made from the rest pose, never from the current state: repeated poses do
 * not drift, a pose after a pt_update_* discards that update's geometry, a later pt_update_* overwrites the pose.
 * The posed arrays then go through what pt_update_meshes runs, so everything on the device is, word for word, what
 * pt_update_meshes with the same arrays computed on the host, normals given, leaves: the world triangle BVH, every
 * BLAS, the meshes' inner boxes, the instances' world boxes, the analytic BVH, the boxes the routed split tests and the
 * lights (a light that is a loose emissive triangle returns to its rest vertices).  An instanced mesh is posed in its
 * object space; its instance matrix stays pt_update_shapes' business, and the two compose in either order.  Runs on the
 * context's stream after every pass issued before it and synchronises before returning; the Buffer, the pass state
 * and the counters are untouched; out_kernel_ms (may be NULL) covers the pose kernel, the normals kernels and the
 * refits.  Non-finite values: boxes (and derived normals) are unspecified; no access leaves its array.
 * Errors (nothing launched, the scene untouched): a NULL ctx, u or matrices, reserved != 0, a normals_mode outside
 * {0, 1, 2}, num_meshes different from the uploaded scene's, no rest pose installed: PT_ERR_INVALID_ARG; no scene:
 * PT_ERR_NO_SCENE; a workspace not allocated: PT_ERR_OUT_OF_MEMORY; PT_NORMALS_SMOOTH with 3 * num_triangles >= 2^31:
 * PT_ERR_UNSUPPORTED.  A scene with no triangle in any BVH: PT_OK, nothing launched. */
typedef struct pt_mesh_pose {
    int32_t num_meshes;        /* must equal the uploaded scene's num_meshes */
    int32_t normals_mode;      /* 0: Mesh.Transform's (MulDirection of the rest normals); PT_NORMALS_FACE; PT_NORMALS_SMOOTH */
    int32_t reserved[2];       /* 0 */
    const double* matrices;    /* [num_meshes][16] row-major, required */
    const int32_t* mesh_mask;  /* [num_meshes] or NULL (= all); 0: the mesh takes its rest values verbatim */
} pt_mesh_pose;
int pt_pose_meshes(void* ctx, const pt_mesh_pose* u, double* out_kernel_ms);
/* The six arrays the last pt_pose_meshes, pt_skin_meshes or pt_morph_meshes left staged on the device (derived normals included), [n][3] each in
 * pt_scene_desc order; any pointer may be NULL.  They stay until a pt_update_* or pt_read_tri_normals reuses the
 * staged arrays.  A NULL ctx, or no pose, skin or morph staged: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_read_pose(void* ctx, float* v1, float* v2, float* v3, float* n1, float* n2, float* n3);

/* Blend skinning on the device: a mesh that bends.  The host sends four bone indices and four weights
 * per corner once (pt_set_skin) and one 4x4 matrix per bone per frame (pt_skin_meshes); the device blends the rest pose
 * pt_set_rest_pose installed, derives or transforms the normals, and refits, as pt_pose_meshes does.
 *
 * pt_set_skin installs the skin: for each of the three corners of every triangle, pt_scene_desc order,
 * PT_SKIN_INFLUENCES (bone index, weight) pairs.  The data is copied to a device workspace of its own (72 B per
 * triangle: the indices are kept in 16 bits; plus 128 B per bone for the matrices) kept until the next pt_upload_scene;
 * a later pt_set_skin replaces it, a later pt_set_rest_pose keeps it.  It needs a scene, not a rest pose, and changes
 * nothing a ray sees.  Weights are not normalised and their values are not checked.  Synchronises before returning.
 * Errors (nothing copied, a previous skin kept): a NULL ctx, desc or array, reserved != 0, num_triangles different from
 * the uploaded scene's, num_bones outside [1, PT_SKIN_MAX_BONES], any of the 12 num_triangles indices outside
 * [0, num_bones), whatever its weight: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the workspace not allocated:
 * PT_ERR_OUT_OF_MEMORY. */
#define PT_SKIN_INFLUENCES 4     /* (bone, weight) pairs per corner */
#define PT_SKIN_MAX_BONES 65536
typedef struct pt_skin_desc {
    int32_t num_triangles;     /* must equal the uploaded scene's num_triangles */
    int32_t num_bones;         /* 1..PT_SKIN_MAX_BONES */
    int32_t reserved[2];       /* 0 */
    const int32_t *bone1, *bone2, *bone3;     /* [num_triangles][4] each: the bones of corner 1, 2, 3; every one in [0, num_bones) */
    const float *weight1, *weight2, *weight3; /* [num_triangles][4] each: their weights; +-0: the influence is dead */
} pt_skin_desc;
int pt_set_skin(void* ctx, const pt_skin_desc* desc);
/* pt_skin_meshes skins the rest pose and refits.  A source triangle belongs to a mesh as for pt_pose_meshes; a loose
 * triangle takes its rest values bit for bit, whatever its weights (a light that is a loose emissive triangle returns
 * to its rest vertices).  For a corner V of a mesh triangle an influence k is live when weight[k] != 0 (false only for
 * +-0; a NaN weight is live).  With no live influence the position, and with normals_mode 0 the normal, take their rest
 * values bit for bit.  Otherwise, over the live k in ascending order, the term is (double)weight[k] * P_k per
 * component, P_k the three fp64 sums Matrix.MulPosition(matrices[bone[k]], V_rest) forms (m[0] x + m[1] y + m[2] z +
 * m[3], left to right) before any conversion; the accumulator is the first live term, each further live term is added
 * to it (it does not start from 0: -0 survives, and a dead influence's matrix is never read); the position is one
 * conversion of the accumulator to fp32.  With normals_mode 0 the normal is blended the same way from
 * Matrix.MulDirection's three fp64 sums (no translation), converted once, then normalised in fp32 as MulDirection ends;
 * with PT_NORMALS_FACE or PT_NORMALS_SMOOTH the normals of every triangle are derived from the skinned positions as
 * pt_update_meshes derives them.  The fourth row of a matrix is not read.  So one live influence of weight 1 gives
 * exactly pt_pose_meshes' result for that bone's matrix.  A skin is always applied to the rest pose, never to the
 * current state: repeated skins do not drift, a later pt_update_* or pt_pose_meshes overwrites the skin and the skin
 * overwrites them.  An instanced mesh is skinned in its object space.  The skinned arrays then go through what
 * pt_update_meshes runs, so everything on the device is, word for word, what pt_update_meshes with the same arrays
 * computed on the host leaves; pt_read_pose returns them, and pt_rebuild_meshes / pt_rebuild_blas with u == NULL take
 * them.  Stream order, the synchronisation, the Buffer, pass state, counters and non-finite values are as for
 * pt_pose_meshes; out_kernel_ms (may be NULL) covers the skin kernel, the normals kernels and the refits.
 * Errors (nothing launched, the scene untouched): a NULL ctx, u or matrices, reserved != 0, a normals_mode outside
 * {0, 1, 2}, num_bones different from the installed skin's, no skin installed, no rest pose installed:
 * PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; a workspace not allocated: PT_ERR_OUT_OF_MEMORY; PT_NORMALS_SMOOTH with
 * 3 * num_triangles >= 2^31: PT_ERR_UNSUPPORTED.  A scene with no triangle in any BVH: PT_OK, nothing launched. */
typedef struct pt_mesh_skin {
    int32_t num_bones;         /* must equal the installed skin's num_bones */
    int32_t normals_mode;      /* 0: the blend of MulDirection of the rest normals; PT_NORMALS_FACE; PT_NORMALS_SMOOTH */
    int32_t reserved[2];       /* 0 */
    const double* matrices;    /* [num_bones][16] row-major, required */
} pt_mesh_skin;
int pt_skin_meshes(void* ctx, const pt_mesh_skin* u, double* out_kernel_ms);
/* The installed skin in pt_skin_desc's form, indices and weight bits as given, [num_triangles][4] each; any pointer may
 * be NULL.  Synchronises and changes nothing.  A NULL ctx, or no skin installed: PT_ERR_INVALID_ARG; no scene:
 * PT_ERR_NO_SCENE. */
int pt_read_skin(void* ctx, int32_t* bone1, int32_t* bone2, int32_t* bone3, float* weight1, float* weight2, float* weight3);

/* Morph targets on the device: faces, muscle bulges and corrective shapes.  A morph target (blend
 * shape) is a sparse set of per-corner offsets; a frame scales each target by one weight and adds it to the rest pose
 * pt_set_rest_pose installed, before the skin.  The host sends the deltas once (pt_set_morph) and 4 bytes per target
 * per frame (pt_morph_meshes), plus 128 bytes per bone when the call also skins.
 *
 * pt_set_morph installs the morph.  Target t owns the deltas target_first[t] .. target_first[t + 1] - 1; delta i moves
 * corner corner[i] = 3 * triangle + c (c = 0, 1, 2 for v1, v2, v3; pt_scene_desc order) by dpos[i] and, when dnrm is
 * given, its normal by dnrm[i].  Within a target the corners ascend strictly (no corner twice); a target may be empty.
 * target_first, corner and dpos are required even when there is no delta.  The data is packed on the host into a
 * sliced ELL format whose slice is one wave (64 consecutive triangles of one corner array; a slice is as long as its
 * busiest corner, the rest is padding) and copied to a device workspace of its own: per step of a slice 128 B of
 * 16-bit target indices and 768 B of position deltas, 768 B more with normal deltas, 12 B per slice, 4 B per target;
 * pt_read_morph's counts[2] is the padded entry count (64 per step), what a sparsity pattern costs.  It is kept
 * until the next pt_upload_scene; a later pt_set_morph replaces it (the new workspace is allocated and filled first,
 * the old one released afterwards), a later pt_set_rest_pose or pt_set_skin keeps it.  It needs a scene, not a rest
 * pose, and changes nothing a ray sees.  Values of deltas are not checked.  Synchronises before returning.
 * Errors (nothing copied, a previous morph kept): a NULL ctx, desc, target_first, corner or dpos, reserved != 0,
 * num_triangles different from the uploaded scene's, num_targets outside [1, PT_MORPH_MAX_TARGETS], target_first[0]
 * != 0 or target_first decreasing, a corner outside [0, 3 * num_triangles) or not above its predecessor in the same
 * target: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the workspace not allocated: PT_ERR_OUT_OF_MEMORY. */
#define PT_MORPH_MAX_TARGETS 65535
typedef struct pt_morph_desc {
    int32_t num_triangles;        /* must equal the uploaded scene's num_triangles */
    int32_t num_targets;          /* 1..PT_MORPH_MAX_TARGETS */
    int32_t reserved[2];          /* 0 */
    const int64_t* target_first;  /* [num_targets + 1], target_first[0] = 0, non-decreasing; the last = number of deltas */
    const int32_t* corner;        /* [deltas]: 3 * triangle + c, c = 0, 1, 2 (pt_scene_desc order); strictly ascending within a target */
    const float*   dpos;          /* [deltas][3] */
    const float*   dnrm;          /* [deltas][3] or NULL: the morph carries no normal deltas */
} pt_morph_desc;
int pt_set_morph(void* ctx, const pt_morph_desc* desc);
/* pt_morph_meshes morphs the rest pose and refits.  A source triangle belongs to a mesh as for pt_pose_meshes; a loose
 * triangle takes its rest values bit for bit whatever deltas name it (a light that is a loose emissive triangle
 * returns to its rest vertices, as after a pose or a skin).  A delta of target t is live when weights[t] != 0 (false
 * only for +-0; a NaN weight is live); a dead delta is skipped by a branch, not multiplied by zero, so a non-finite
 * delta of a dead target changes nothing.  A corner of a mesh triangle with no live delta is copied bit for bit,
 * position and normal.  Otherwise, per component, a = (double)p, the rest value, then over the corner's live deltas in
 * ascending target order a = a + (double)weights[t] * (double)d; the position is one conversion of a to fp32.  The
 * product of two widened floats is exact in fp64, so the result does not depend on whether the multiply and the add
 * are contracted (the build keeps -ffp-contract=off anyway).  Normals: with normals_mode 0 and a morph that carries
 * dnrm, the normal is accumulated the same way from the rest normal and dnrm, converted once, then normalised by the
 * fp32 Normalize Matrix.MulDirection ends in (a zero-length result is NaN, as Normalize gives); with normals_mode 0
 * and no dnrm the rest normals are copied; with PT_NORMALS_FACE or PT_NORMALS_SMOOTH the normals of every triangle
 * are derived from the morphed positions as pt_update_meshes derives them.  A morph is always made from the rest pose,
 * never from the current state: repeated morphs do not drift, a later pt_update_*, pt_pose_meshes or pt_skin_meshes
 * overwrites the morph and the morph overwrites them.  An instanced mesh is morphed in its object space.
 * With skin_matrices the call composes the two deformers: the morphed six arrays (normals as normals_mode 0 gives them
 * above; with PT_NORMALS_FACE or PT_NORMALS_SMOOTH the rest normals are carried) go to an intermediate device buffer
 * (72 B per triangle, allocated by the first such call and kept until the next pt_upload_scene), and pt_skin_meshes'
 * kernel blends that buffer in place of the rest pose, with the same normals_mode: the result is skin(morph(rest))
 * exactly.  It needs a skin installed (pt_set_skin) and num_bones equal to the installed skin's; without
 * skin_matrices num_bones is 0.
 * The arrays then go through what pt_update_meshes runs, so everything on the device is, word for word, what
 * pt_update_meshes with the same arrays computed on the host leaves; pt_read_pose returns them, and pt_rebuild_meshes /
 * pt_rebuild_blas with u == NULL take them.  Stream order, the synchronisation, the Buffer, pass state, counters and
 * non-finite values are as for pt_pose_meshes; out_kernel_ms (may be NULL) covers the morph kernel, the skin kernel,
 * the normals kernels and the refits.
 * Errors (nothing launched or copied, the scene untouched): a NULL ctx, u or weights, reserved != 0, a normals_mode
 * outside {0, 1, 2}, no morph installed, num_targets different from the installed morph's, num_bones != 0 without
 * skin_matrices, skin_matrices with no skin installed or num_bones different from the installed skin's, no rest pose
 * installed: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; a workspace not allocated: PT_ERR_OUT_OF_MEMORY;
 * PT_NORMALS_SMOOTH with 3 * num_triangles >= 2^31: PT_ERR_UNSUPPORTED.  A scene with no triangle in any BVH: PT_OK,
 * nothing launched. */
typedef struct pt_mesh_morph {
    int32_t num_targets;          /* must equal the installed morph's */
    int32_t normals_mode;         /* 0, PT_NORMALS_FACE, PT_NORMALS_SMOOTH */
    int32_t num_bones;            /* 0 when skin_matrices is NULL, else the installed skin's */
    int32_t reserved;             /* 0 */
    const float*  weights;        /* [num_targets], required */
    const double* skin_matrices;  /* NULL: morph only; else [num_bones][16]: morph, then pt_skin_meshes' blend of the morphed pose */
} pt_mesh_morph;
int pt_morph_meshes(void* ctx, const pt_mesh_morph* u, double* out_kernel_ms);
/* The installed morph in pt_morph_desc's form, bit for bit: counts receives the targets, the deltas and the padded
 * entries held on the device; target_first [targets + 1], corner [deltas], dpos and dnrm [deltas][3].  The packed
 * device data is read back and unpacked on the host, so this is what the device holds.  Any pointer but ctx may be
 * NULL (call once for counts, then with arrays); dnrm is written only when the morph carries normal deltas.
 * Synchronises and changes nothing.  A NULL ctx, or no morph installed: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_read_morph(void* ctx, int64_t counts[3] /* targets, deltas, padded entries held on the device */,
                  int64_t* target_first, int32_t* corner, float* dpos, float* dnrm);

/* Re-sorting the world triangle BVH on the device.  The updates above refit: they keep the topology
 * of the pose the tree was built for, and a mesh deformed far from it traces an ever worse tree.  pt_rebuild_meshes
 * takes pt_update_meshes' struct and does everything that call does (positions; normals given, kept or derived), and
 * in addition replaces the topology of the world triangle BVH (loose triangles and top-level meshes together) by a
 * balanced object-median tree for these positions: with P triangles in the BVH, chunks of three consecutive positions,
 * h = the least integer >= 1 with 3 * 8^h >= P levels of nodes that group 8 consecutive chunks, then 8 consecutive nodes,
 * numbered level by level from the root; the order comes from 3 h rounds of stable sorts of ever halved position
 * segments by the key min + max of the triangle's vertices on the segment's widest axis (pt_rebuild.h states it
 * exactly).  The tree's shape depends on P alone, the order is computed on the device, and every box, record and chunk
 * line then comes from the refit.  With u == NULL the arrays the last pt_pose_meshes or pt_skin_meshes left staged are taken: nothing is
 * copied, the staged normals are used and the pose or skin stays readable.
 * Afterwards every ray query, feature pass and render pass sees what a fresh pt_upload_scene with these arrays would
 * see, up to the exact-t tie order of DESIGN.md §5, and every later pt_update_triangles, _normals, pt_update_meshes,
 * pt_pose_meshes, pt_read_tri_normals and pt_read_tri_bvh works on the new topology (pt_read_tri_bvh's counts follow;
 * lines past them are left as they are, nothing references them).  The lights that are loose emissive triangles follow.
 * pt_stats' bvh_nodes, bvh_bytes and traversal_bytes keep describing the upload.  The process-wide build cache is
 * untouched: other contexts keep their trees.  Runs on the context's stream after every pass issued before it and
 * synchronises before returning; out_kernel_ms (may be NULL) covers every kernel of the call.  Non-finite positions:
 * the order is unspecified, still a permutation; no access leaves its array.
 * Errors (nothing launched, the scene untouched): those of pt_update_meshes (u == NULL without a staged pose or skin:
 * PT_ERR_INVALID_ARG); a scene with an instanced mesh, whose BLAS is not rebuilt: PT_ERR_UNSUPPORTED (pt_rebuild_blas
 * below serves such a scene); more than 9 levels, or more node and chunk lines together than the upload allocated
 * (nodes and chunks share one run of lines,
 * so a tree with more nodes than the uploaded one starts its chunks later; short only when the uploaded tree was
 * within a few lines of perfectly full): PT_ERR_UNSUPPORTED; the workspace (about 130 B per triangle, kept until the
 * next upload) not allocated: PT_ERR_OUT_OF_MEMORY.  A scene with no triangle in the BVH: PT_OK, nothing launched. */
int pt_rebuild_meshes(void* ctx, const pt_mesh_update* u, double* out_kernel_ms);
/* The surface-area cost of the world triangle BVH from the node words as they stand, valid any time after an upload:
 * every slot box decoded in fp64 as origin + q 2^(e - 127), A = the area of the union of the root's slot boxes;
 * out[0] = (A + the area of every inner slot) / A, out[1] = the area of every leaf slot / A, out[2] = A.  Summed on
 * the device.  No triangle in the BVH (or A == 0): zeros.  Synchronises and changes nothing.  A NULL argument:
 * PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_tri_bvh_cost(void* ctx, double out[3]);

/* Re-sorting instanced meshes' BLASes on the device.  pt_rebuild_blas takes pt_update_meshes' struct and
 * does everything that call does (positions; normals given, kept or derived; u == NULL: the staged pose or skin, as
 * pt_rebuild_meshes takes it), and re-sorts what `what` names: PT_REBUILD_WORLD the world triangle BVH, exactly as
 * pt_rebuild_meshes does (its refusals for too many levels or lines included; on a scene without an instanced mesh the
 * device then holds, word for word, what pt_rebuild_meshes leaves), PT_REBUILD_BLAS every BLAS, 0 both.  A BLAS of n
 * triangles gets a balanced object-median BVH4 whose shape depends on n alone: leaves of four consecutive positions,
 * h = the least integer >= 1 with 4 * 4^h >= n levels of nodes that group 4 consecutive leaves, then 4 consecutive nodes,
 * numbered level by level from the root; the order comes from 2 h rounds of stable sorts of ever halved position
 * segments, by pt_rebuild_meshes' key and axis rule (pt_blas_rebuild.h states it exactly).  Then pt_update_meshes' BLAS
 * refit and pt_update_shapes' refit run over the new order.  A BLAS whose balanced tree needs more nodes than the upload
 * gave it is refitted, not rebuilt: it keeps its topology and order, the call still succeeds.  pt_read_blas' node count
 * of a rebuilt BLAS becomes the new tree's and stays for a kept one; counts[1] and every offset stay, lines past a
 * BLAS's new count are left as they are.  A scene whose only triangles are instanced launches nothing for the world.
 * Afterwards every ray query, feature pass and render pass sees what a fresh pt_upload_scene with these arrays and the
 * current shape parameters would see, up to the exact-t tie order of DESIGN.md §5; pt_intersect_hits' identities stay
 * the source numbering; every later pt_update_meshes, pt_pose_meshes and pt_read_blas works on the new topology.
 * Stream order, synchronisation, out_kernel_ms, the Buffer, pass state, counters and non-finite inputs are as for
 * pt_rebuild_meshes.  PT_BLAS_TAIL in the environment, read at each call, sizes the segments one workgroup finishes in
 * LDS (0: none, every round a device sort; else the largest 4 * 4^k in [64, 1024] it holds); the words left on the
 * device do not depend on it.
 * Errors (nothing launched, the scene untouched): those of pt_update_meshes (u == NULL without a staged pose or skin:
 * PT_ERR_INVALID_ARG); `what` outside 0..3: PT_ERR_INVALID_ARG; a BLAS of more than 10 levels: PT_ERR_UNSUPPORTED; a
 * workspace (about 100 B per BLAS triangle, kept until the next upload) not allocated: PT_ERR_OUT_OF_MEMORY. */
#define PT_REBUILD_WORLD 1 /* what pt_rebuild_meshes re-sorts */
#define PT_REBUILD_BLAS 2  /* every BLAS */
int pt_rebuild_blas(void* ctx, const pt_mesh_update* u, int32_t what, double* out_kernel_ms);
/* pt_tri_bvh_cost for each BLAS, from the BVH4 node words as they stand (plain fp32 child boxes, widened to fp64):
 * with A = the area of the union of the root's slot boxes, out[3 b] = (A + the area of every inner slot) / A,
 * out[3 b + 1] = the area of every leaf slot / A, out[3 b + 2] = A; A == 0: zeros.  Summed on the device, per BLAS in a
 * fixed order.  num_blas must equal pt_read_blas' counts[0].  Synchronises and changes nothing.  A NULL argument or a
 * wrong count: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_blas_cost(void* ctx, int32_t num_blas, double* out /* [num_blas][3] */);

/* New voxels and new iso-windows for the Volumes of the uploaded scene: what a user edits
 * interactively (an iso-window dragged to another tissue, the next grid of a time series), without the re-upload
 * that recompiles and re-sends the whole scene.  data[i] non-NULL gives volume i new voxels, [d][h][w] doubles of
 * the uploaded dimensions; windows[i] non-NULL gives it new lo and hi for each of its uploaded num_windows windows
 * (the materials must equal the uploaded ones).  Volumes are in pt_scene_desc order; the arrays are copied during
 * the call.
 * Equivalence: afterwards every ray query, feature pass and render pass sees the scene a fresh pt_upload_scene of
 * the same pt_scene_desc with these voxels and windows substituted would see, and every word of the volume state on
 * the device equals that upload's: the voxels, the window rows, the uniform-cell signs of the march skip (1 B per
 * cell of the (w+1)(h+1)(d+1) lattice), the cell-major corners (64 B per cell) where the upload made them, and the
 * header's zero_sign.  No tie-order caveat: nothing is re-sorted.  The dimensions, zscale, the box, the window
 * count and the materials stay, and with them what the upload decided from them: which volumes have cell-major
 * corners, the LDS staging of a scene's one Volume, the routing and every BVH (the box is given, not derived from
 * the voxels, so no box, record or light sphere moves).  A Volume reached through a pt_transformed_shape is served
 * too: that shape reads the same volume.  New dimensions, zscale, box, window count or window materials need a
 * pt_upload_scene.
 * Rebuild scope: a volume given new data has its voxels copied in and both tables rebuilt on the device from them;
 * a volume given only new windows has its window rows, its signs and zero_sign rebuilt, and its voxels are neither
 * sent nor copied (24 B per window cross the bus).
 * Lights: Scene.Add registers a shape as a light when MaterialAt(origin).Emittance > 0 (Scene.cs:29-38).  For a
 * Volume, and for a TransformedShape over one (whose MaterialAt passes the point on unmapped), that is the material
 * of the sample at the origin, which is 0 whatever the voxels (Sample's z index there is d, past the last slice), so
 * it depends on the windows alone.  This call does not change the set of lights (the upload's, or the one the last
 * pt_update_materials left): before anything is copied or launched it evaluates the test with the new windows and
 * refuses with PT_ERR_UNSUPPORTED when any shape's membership in the current set would differ.  A light that stays one takes the material the test now gives.
 * Ordering: runs on the context's stream after every pass issued before it and synchronises before returning.  The
 * Buffer, the pass state, the counters, the feature buffers, the query tables and the process-wide build cache are
 * untouched.  out_kernel_ms (may be NULL) is the device time of the call's kernels.
 * Non-finite voxels, lo and hi behave as at upload: a cell with a non-finite corner is "cannot vouch" (sign 0); no
 * access leaves its array.
 * Errors (nothing launched, the scene untouched): a NULL ctx or u, reserved != 0, num_volumes different from the
 * scene's, a window's material different from the uploaded one: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; a
 * changed light membership: PT_ERR_UNSUPPORTED.  Both arrays NULL, every entry NULL, or a scene without volumes and
 * num_volumes 0: PT_OK, nothing launched, *out_kernel_ms = 0. */
typedef struct pt_volume_update {
    int32_t num_volumes;                       /* must equal the uploaded scene's */
    int32_t reserved[3];                       /* 0 */
    const double* const * data;                /* NULL, or [num_volumes]: data[i] NULL = volume i keeps its voxels,
                                                  else [d][h][w] doubles of the uploaded dimensions */
    const pt_volume_window* const * windows;   /* NULL, or [num_volumes]: windows[i] NULL = kept, else the uploaded
                                                  num_windows entries; lo and hi are taken, material must equal the uploaded one */
} pt_volume_update;
int pt_update_volumes(void* ctx, const pt_volume_update* u, double* out_kernel_ms);
/* What the device holds for volume `index` (tests and tools): info = {w, h, d, num_windows, zero_sign, has_cells,
 * cells in the table = (w+1)(h+1)(d+1), 0}; data receives w h d doubles, windows num_windows entries, runs one int8
 * per cell, cells 8 doubles per cell when has_cells (else it is left alone).  Every pointer but ctx may be NULL.
 * Synchronises and changes nothing.  A NULL ctx, or an index outside the scene's volumes: PT_ERR_INVALID_ARG; no
 * scene: PT_ERR_NO_SCENE. */
int pt_read_volume(void* ctx, int32_t index, int64_t info[8], double* data, pt_volume_window* windows,
                   int8_t* runs, double* cells);

/* New materials and a new environment for the uploaded scene: a light dimmed, a material recoloured,
 * an emitter switched on, the environment map turned or swapped, without the re-upload that recompiles both BVHs and
 * re-sends the geometry.  materials non-NULL replaces every row of the material table; flags & PT_LOOK_ENV takes
 * env_color, env_texture and env_texture_angle (else the environment stays).  The arrays are copied during the call.
 * Equivalence: afterwards every ray query, feature pass and render pass sees what a fresh pt_upload_scene of the same
 * pt_scene_desc with these materials and environment values substituted, and the geometry the device holds now,
 * would see; every word of the material table and of the light table, num_lights, lights_lean, route and
 * shade_route equal that upload's.  No tie-order caveat: nothing is re-sorted.  Which material a shape uses (the
 * *_material arrays, window and SDF materials), the number of materials and the number and size of the textures
 * stay; changing those needs a pt_upload_scene.
 * Lights follow: Scene.Add makes a shape a light when MaterialAt(origin).Emittance > 0 (Scene.cs:29-38), so with new
 * emittances the set of lights may grow, shrink or reorder; the call runs the upload's own light and flag
 * derivation on the new table and the shapes' current parameters (a light's sphere comes from where pt_update_shapes,
 * pt_update_triangles, pt_update_meshes or pt_pose_meshes left its shape), and the later updates move the lights of
 * the new list.  pt_update_volumes tests light membership against the set this call left.  The device light array
 * grows once to num_shapes entries when the list outgrows the upload's (PT_ERR_OUT_OF_MEMORY before anything
 * changes if it cannot).
 * Ordering: runs on the context's stream after every pass issued before it and synchronises before returning.
 * Everything is validated and derived on the host before the first copy.  The Buffer, the pass state, the counters,
 * the feature buffers, the query tables and the build cache are untouched.  out_kernel_ms (may be NULL) is 0: the
 * call launches no kernel.
 * Errors (nothing copied, the scene untouched): a NULL ctx or u, reserved != 0, flags outside {0, PT_LOOK_ENV},
 * materials given with num_materials different from the scene's, a texture slot of a material or of the environment
 * outside [0, num_textures]: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE.  materials NULL and no flag: PT_OK,
 * nothing done.  Values are not range-checked, as at upload.  A copy that fails after the checks is PT_ERR_HIP, as
 * in the other updates: the device's tables are then part old, part new, and the context needs a pt_upload_scene. */
#define PT_LOOK_ENV 1                 /* flags: the env_* fields are taken; else the environment stays */
typedef struct pt_material_update {
    int32_t num_materials;            /* must equal the uploaded scene's */
    int32_t flags;                    /* 0 or PT_LOOK_ENV */
    int32_t reserved[2];              /* 0 */
    const pt_material* materials;     /* [num_materials], or NULL = kept */
    double  env_color[3];             /* Scene.Color */
    int32_t env_texture, _pad;        /* Scene.Texture, 1-based, 0 = null, <= the uploaded num_textures */
    double  env_texture_angle;        /* Scene.TextureAngle */
} pt_material_update;
int pt_update_materials(void* ctx, const pt_material_update* u, double* out_kernel_ms);
/* What the device holds now (tests and tools).  info: the counts, the flags the passes are planned from and the
 * environment; materials receives num_materials rows, texture slots 1-based again, read back from the device;
 * light_rows receives per light {kind (DevLight: 0 sphere, 1 cube, 2 plane, 3 triangle, 5 SDF, 6 Volume, 7
 * transformed), index, material, phantom}, light_spheres per light {centre x, y, z widened to double, radius},
 * both in the lights' order and read back from the device (a scene has at most num_shapes lights).  Every pointer but
 * ctx may be NULL.  Synchronises and changes nothing.  A NULL ctx: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
typedef struct pt_look_info {
    int32_t num_materials, num_textures, num_lights;
    int32_t lights_lean, route, shade_route;   /* DevScene's flags */
    int32_t env_texture, _pad;                 /* 1-based, 0 = null */
    double env_color[3];
    double env_texture_angle;
} pt_look_info;
int pt_read_materials(void* ctx, pt_look_info* info, pt_material* materials, int32_t* light_rows, double* light_spheres);

/* New texels for the textures of the uploaded scene: the next frame of a video texture, a swapped
 * image.  images[i] non-NULL gives texture i new texels of the uploaded width and height.  PT_TEXELS_F64 is a copy
 * into place of [h][w][3] doubles, as pt_texture::data.  The 8-bit formats send the image's bytes and a 256-entry
 * table: a texture made from an 8-bit image is (byte / 255)^2.2 per channel (ColorTexture.NewTexture,
 * Texture.cs:150-166), and ITexture.Pow and MulScalar map every texel through one function, so every texel channel is
 * lut[byte].  The host computes the table with its own pow, the bit patterns it would have sent; the device
 * (k_tex_decode, pt_texture.hip) looks the bytes up and writes the doubles, and never calls pow: the texels are
 * bit-equal to the F64 route by construction, for 3 or 4 bytes per texel over the bus instead of 24.
 * Equivalence: the texel words equal a fresh upload's with the host-decoded pt_texture; everything else is
 * untouched (ordering and scope as pt_update_materials).  out_kernel_ms (may be NULL): the decode kernels' device
 * time, 0 when none ran.
 * Errors (nothing copied, the scene untouched): a NULL ctx or u, reserved != 0, num_textures different from the
 * scene's, an image whose width or height differ from the uploaded texture's, a format outside the enum, a NULL data
 * in a non-NULL image, a NULL lut with an 8-bit format: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the byte
 * staging (4 B per texel of the scene plus the tables, kept until the next upload) not allocated:
 * PT_ERR_OUT_OF_MEMORY.  images NULL or every entry NULL: PT_OK, nothing launched. */
typedef enum pt_texel_format { PT_TEXELS_F64 = 0, PT_TEXELS_RGB8 = 1, PT_TEXELS_RGBA8 = 2 } pt_texel_format;
typedef struct pt_texture_image {
    int32_t width, height;            /* must equal the uploaded texture's */
    int32_t format, reserved;         /* pt_texel_format; 0 */
    const void*   data;               /* F64: [h][w][3] double; RGB8 / RGBA8: [h][w][3|4] bytes, rows packed, A ignored */
    const double* lut;                /* [256], required for the 8-bit formats: texel channel = lut[byte] */
} pt_texture_image;
typedef struct pt_texture_update {
    int32_t num_textures;             /* must equal the uploaded scene's */
    int32_t reserved[3];              /* 0 */
    const pt_texture_image* const * images;  /* NULL, or [num_textures]; a NULL entry = that texture stays */
} pt_texture_update;
int pt_update_textures(void* ctx, const pt_texture_update* u, double* out_kernel_ms);
/* The texels the device holds for texture `index` (tests and tools): info = {width, height, 0, 0}; data receives
 * [h][w][3] doubles.  info and data may be NULL.  A NULL ctx or an index outside the scene's textures:
 * PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE. */
int pt_read_texture(void* ctx, int32_t index, int32_t info[4], double* data);

/* ---- Motion vectors and temporal accumulation across animated frames.
 * One animated frame on the host: apply the frame's updates; pt_reset_buffer and render passes (pass numbers keep
 * counting across frames); pt_render_motion(cam); pt_accumulate_temporal; pt_denoise_temporal and pt_read_denoised;
 * pt_motion_snapshot(cam).  The first frame runs the same sequence.
 *
 * pt_motion_snapshot records "the previous frame": the camera, and device-to-device copies of the geometry as the
 * device holds it now: every world and BLAS triangle record {v1, e1, e2} stored at its source triangle (so a later
 * rebuild's re-sort does not matter), the analytic records, the instance matrices and the instances' inner records
 * (those three by record position: nothing re-sorts them).  The storage is context-owned, allocated on first use
 * and dropped by the next pt_upload_scene together with the motion result and the history.  It ensures the identity
 * tables as the scene's first pt_intersect_hits does, and changes no Buffer, pass state, features or counters.
 * A NULL ctx or camera: PT_ERR_INVALID_ARG; no scene: PT_ERR_NO_SCENE; the storage not allocated:
 * PT_ERR_OUT_OF_MEMORY, the previous snapshot kept. */
int pt_motion_snapshot(void* ctx, const pt_camera* camera);

/* One primary ray per pixel as pt_render_features casts it (Camera.CastRay(x, y, W, H, 0.5, 0.5), the lens ignored),
 * and per pixel what pt_read_motion returns.  The previous position of the hit point is defined per kind of shape in
 * ptsharp_amd/csrc/pt_motion.h, in fp64.  Without a snapshot on the context (status 2) shape, prim and depth are still
 * written, so frame 0 runs the same sequence.  Errors as pt_motion_snapshot. */
int pt_render_motion(void* ctx, const pt_camera* camera, double* out_kernel_ms);

typedef enum pt_motion_array {
    PT_MOTION_SHAPE_I32 = 0,      /* [H][W] int32: pt_intersect_hits' `shape` for the pixel's ray; -1 on a miss */
    PT_MOTION_PRIM_I32 = 1,       /* [H][W] int32: its `prim`; -1 on a miss */
    PT_MOTION_DEPTH_F64 = 2,      /* [H][W] double: the hit's t, or 1e9 on a miss */
    PT_MOTION_PREV_XY_F64 = 3,    /* [H][W][2] double: the previous frame's continuous pixel coordinates of the same
                                     surface point; (-1, -1) behind the previous camera, not finite, or without snapshot */
    PT_MOTION_PREV_DEPTH_F64 = 4, /* [H][W] double: that point's distance from the previous camera; 1e9 for a miss */
    PT_MOTION_PREV_PIXEL_I32 = 5, /* [H][W] int32: the nearest previous pixel floor(x' + 0.5) + W·floor(y' + 0.5), or -1 */
    PT_MOTION_STATUS_I32 = 6      /* [H][W] int32: 0 ok; 1 outside the previous image, behind the previous camera or not
                                     finite; 2 no snapshot on the context */
} pt_motion_array;
/* One array of the last pt_render_motion, row-major, into the caller's `out`.  A NULL ctx or out, `what` outside the
 * enum, or no motion result on the context: PT_ERR_INVALID_ARG. */
int pt_read_motion(void* ctx, int32_t what, void* out);

/* max_history: the samples the history may weigh at most, 0..2^20; sigma_depth: the relative depth tolerance, finite
 * and >= 0, 0 switches the depth test off.  NULL = 32 and 0.1: design defaults, not tuned values. */
typedef struct pt_temporal_params {
    int32_t max_history;
    int32_t reserved;     /* 0 */
    double sigma_depth;
} pt_temporal_params;

/* Merges the history into the current Buffer's statistics.  For pixel p with q = prev_pixel[p] the status is the first
 * that applies: 7 the current pixel is invalid (pt_denoise's rule; a tile-sharded context's foreign pixels, N = 0);
 * 1 no history; 2 the motion status is not 0; 3 the history at q is invalid; 4 (shape, prim) at p differs from the
 * history's at q; 5 |prev_depth[p] − hist_depth[q]| > sigma_depth·prev_depth[p]; 0 merged.  On any status but 0 the
 * temporal pixel is the Buffer's pixel as it stands; on 0 it is Chan's pairwise update in fp64 per channel with
 * Nh' = min(Nh, max_history) (clamped so that Nc + Nh' fits int32; Nh' = 0 leaves the Buffer's pixel):
 *   Vh' = Nh >= 2 ? Vh·((Nh' − 1)/(Nh − 1)) : Vh;  N = Nc + Nh';  δ = Mh − Mc;
 *   M = Mc + δ·(Nh'/N);  V = Vc + Vh' + (δ·δ)·(Nc·Nh'/N).
 * The result {M, V, N, status} is context-owned (pt_read_temporal); with this frame's (shape, prim, depth) it becomes
 * the history, which is double-buffered: the merge reads one set and writes the other.  Changes neither the Buffer nor
 * the pass state nor the features.  Lighting and material changes are not detected: call pt_reset_temporal after them.
 * Needs a motion result rendered since the last pt_accumulate_temporal or pt_reset_temporal.  That missing, a NULL ctx,
 * or a field out of range: PT_ERR_INVALID_ARG, nothing launched; the storage not allocated: PT_ERR_OUT_OF_MEMORY. */
int pt_accumulate_temporal(void* ctx, const pt_temporal_params* params, double* out_kernel_ms);
/* The last pt_accumulate_temporal's result: m, v [H][W][3] double, n, status [H][W] int32; each may be NULL.
 * A NULL ctx or no temporal result on the context: PT_ERR_INVALID_ARG. */
int pt_read_temporal(void* ctx, double* m, double* v, int32_t* n, int32_t* status);
/* pt_denoise (`plain`, or both NULL for its defaults) or pt_denoise_guided (`guided`; the context needs features) on
 * the temporal {M, V, N} instead of the Buffer.  The result goes where pt_denoise's goes.  Both params non-NULL, or no
 * temporal result on the context: PT_ERR_INVALID_ARG; else the errors of the filter called. */
int pt_denoise_temporal(void* ctx, const pt_denoise_params* plain, const pt_denoise_guided_params* guided, double* out_kernel_ms);
/* Drops the history and the temporal and motion results and keeps the snapshot: after a cut, or after
 * pt_update_materials or another change of the lighting.  A NULL ctx: PT_ERR_INVALID_ARG. */
int pt_reset_temporal(void* ctx);

/* Instrumentation (bench / roofline): last pass' traversal counters, summed. */
typedef struct pt_trace_counters {
    uint64_t rays;            /* all Scene.Intersect calls                     */
    uint64_t nodes_visited;   /* BVH child-pair fetches (64 B each), all rays  */
    uint64_t prims_tested;    /* triangle/sphere/cube records tested (48 B)     */
    uint64_t shading_fetches; /* closest-hit shading records (40 B)            */
    uint64_t shadow_rays;     /* the shadow-visibility part of the above ...   */
    uint64_t shadow_nodes;
    uint64_t shadow_prims;
    uint64_t lit_shadow_rays; /* shadow rays whose light was the nearest hit (terms added)   */
    uint64_t accum_runs;      /* their per-pixel runs after wave aggregation (atomic sets)  */
    uint64_t volume_samples;  /* Volume.Sample calls of Volume.Intersect's march (Volume.cs:168-197) */
    uint64_t sdf_evals;       /* SDF evaluations of SDFShape.Intersect's sphere tracing (SDF.cs:32-76) */
    /* The cooperative Volume march's time by phase, shader-clock cycles summed over the marching waves
     * (s_memtime around each phase, so they run ~10 % slower in a counted pass): [0] strided passes over
     * uniform cells, [1] a dense round's position and uniform-cell table read, [2] its corner reads and
     * interpolation, [3] its window loop (Volume.Sign), [4] its ballots and bookkeeping, [5] refinements;
     * [6] dense rounds, [7] strided-pass rounds (counts). */
    uint64_t march_clock[8];
} pt_trace_counters;
int pt_render_pass_counted(void* ctx, const pt_camera* camera, const pt_sampler* sampler,
                           const pt_pass_params* pass, pt_trace_counters* out);

#ifdef __cplusplus
}
#endif
#endif /* PTSHARP_HIP_H */
