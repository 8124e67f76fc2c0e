/* lumo_amd: MI355X (gfx950) wavefront path tracer behind a C ABI.
 *
 * This header is the drop-in boundary for lumo's render hot path (ekarpp/lumo v0.6.1).
 * Every entry point names the reference interface it replaces (paths relative to the
 * lumo source tree).  Plain C: fixed-width integers, doubles, pointers and sizes only.
 * All calls return lumo_status (0 = OK); no exceptions cross the ABI.  A context is
 * bound to one GPU and owns all of its state (device buffers, streams, options, timers):
 * contexts share nothing mutable, so different contexts, on the same GPU or on different
 * ones, may be driven concurrently from different host threads; one context is used by one
 * thread at a time.
 */
#ifndef LUMO_AMD_H
#define LUMO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUMO_ABI_VERSION 10

typedef int32_t lumo_status;
enum {
    LUMO_OK = 0,
    LUMO_ERR_INVALID = 1,     /* bad argument / malformed scene            */
    LUMO_ERR_NO_DEVICE = 2,   /* HIP device missing or not gfx950           */
    LUMO_ERR_HIP = 3,         /* HIP runtime error                          */
    LUMO_ERR_NO_SCENE = 4,    /* render/trace before lumo_scene_upload      */
    LUMO_ERR_NO_CAMERA = 5,   /* render before lumo_camera_set              */
    LUMO_ERR_UNSUPPORTED = 6, /* feature outside the implemented scope      */
    LUMO_ERR_OOM = 7
};

/* ---------------------------------------------------------------------------------
 * Flattened scene (the device image of lumo's Scene, src/tracer/scene.rs:17-29).
 * Produced on the host by lumo_amd's scene builder (or by lumo's own Rust Scene after
 * build(): the arrays below are exactly its BVH / kd-tree node arrays), copied to HBM
 * by lumo_scene_upload.  The caller owns all host arrays.
 * ------------------------------------------------------------------------------- */

/* Spectrum as sigmoid polynomial, f32 (spectrum.rs:14-19). */
typedef struct {
    float c0, c1, c2, scale;
} lumo_spectrum;

enum {
    LUMO_MAT_BLANK = 0,
    LUMO_MAT_LAMBERTIAN = 1,   /* BxDF::Lambertian (bxdf/scatter.rs:3-27)          */
    LUMO_MAT_LIGHT = 2,        /* Material::Light (material.rs:15, 223-234)         */
    LUMO_MAT_MF_DIFFUSE = 3,   /* BxDF::MfDiffuse    (bxdf/microfacet.rs:120-199)    */
    LUMO_MAT_MF_CONDUCTOR = 4, /* BxDF::MfConductor  (bxdf/microfacet.rs:62-118)     */
    LUMO_MAT_MF_DIELECTRIC = 5 /* BxDF::MfDielectric (bxdf/microfacet.rs:201-374)    */
};
enum { LUMO_MATF_CONSTANT_ETA = 1 /* DenseSpectrum::is_constant of eta (no dispersion) */ };

/* Textures (texture.rs:23-92, image.rs).  A material's albedo / ks / tf slot is its solid
 * spectrum when the slot's texture index is -1, else textures[index] evaluated at the hit's uv. */
enum {
    LUMO_TEX_SOLID = 0,        /* Texture::Solid                                        */
    LUMO_TEX_IMAGE = 1,        /* Texture::Image (image.rs:99-128, 170-184): texels[first..]  */
    LUMO_TEX_CHECKERBOARD = 2, /* Texture::Checkerboard(first, second, scale)           */
    LUMO_TEX_MARBLE = 3,       /* Texture::Marble(perlin[first], spec)                  */
    LUMO_TEX_MANDELBROT = 4    /* Texture::Mandelbrot                                   */
};
typedef struct {
    int32_t kind;          /* LUMO_TEX_*                                                 */
    int32_t width, height; /* IMAGE                                                      */
    int32_t first;         /* IMAGE: first texel; CHECKERBOARD: even cells; MARBLE: perlin */
    int32_t second;        /* CHECKERBOARD: odd cells                                    */
    int32_t pad0;
    double scale;          /* CHECKERBOARD                                               */
    lumo_spectrum spec;    /* SOLID / MARBLE colour; IMAGE: mean (Texture::power)        */
} lumo_texture;
/* Image<Normal> bump map (image.rs:131-166): normal_texels[3 * (first + x + y * width)..] */
typedef struct {
    int32_t width, height, first, pad0;
} lumo_normal_map;
/* Perlin noise lattice (perlin.rs): 256 unit normals and the x / y / z permutations */
typedef struct {
    double lattice[256][3];
    int32_t perm[3][256];
} lumo_perlin;

typedef struct {
    int32_t kind;       /* LUMO_MAT_*                                           */
    int32_t two_sided;  /* Light: emits from the back face too                   */
    int32_t illuminant; /* Light: index into dense_spectra                       */
    int32_t eta_idx;    /* microfacet: dense_spectra index of eta                */
    int32_t k_idx;      /* microfacet: dense_spectra index of k                  */
    int32_t flags;      /* LUMO_MATF_*                                           */
    double scale;       /* Light: emission scale                                 */
    double roughness;   /* microfacet: max(roughness, 1e-5)                      */
    lumo_spectrum albedo; /* Lambertian spectrum / Light texture / microfacet kd  */
    lumo_spectrum ks;
    lumo_spectrum tf;
    /* texture indices of albedo / ks / tf (-1: the solid spectrum above) and the bump map
     * (-1: none) of Material::Standard (material.rs:323-331) */
    int32_t albedo_tex, ks_tex, tf_tex, normal_map;
} lumo_material;

/* lumo BVH node (object/bvh.rs:18-26, bvh/node.rs:8-14), depth-first layout:
 * left child = index + 1, `right` = index of the right child or -1.
 * A leaf has count > 0: items[first .. first+count) are object indices. */
typedef struct {
    double bmin[3], bmax[3];
    int32_t right;
    int32_t first;
    int32_t count;
    int32_t pad0;
} lumo_bvh_node;

/* lumo kd-tree node (object/kdtree/node.rs:24-31), pre-order layout:
 * left child = index + 1; leaf: items[first .. first+count) are triangle indices
 * local to the owning object. */
typedef struct {
    double point;
    int32_t axis;
    int32_t right;
    int32_t leaf;
    int32_t first;
    int32_t count;
    int32_t pad0;
} lumo_kd_node;

enum {
    LUMO_OBJ_KDMESH = 0,    /* KdTree<Triangle> (TriangleMesh::new, triangle_mesh.rs:46-60) */
    LUMO_OBJ_RECTANGLE = 1, /* Rectangle (object/rectangle.rs): 2-triangle kd mesh + uv/sampling */
    LUMO_OBJ_TRIANGLE = 2,  /* a single Triangle (object/triangle.rs), e.g. an emissive OBJ face
                               added as a light (parser/obj.rs:93-103)                       */
    LUMO_OBJ_SPHERE = 3     /* Sphere at the local origin (object/sphere.rs), e.g. the
                               environment light of Scene::build (scene.rs:33-52)            */
};

/* Instance transform (object/instance.rs, math/transform.rs): row-major 4x4 local->world `m`,
 * its inverse `inv`, and the normal transform (transpose of inv's 3x3, Transform::to_normal). */
typedef struct {
    double m[16];
    double inv[16];
    double nrm[9];
    double pad0;
} lumo_transform;

typedef struct {
    int32_t type;      /* LUMO_OBJ_* of the shape                        */
    int32_t material;  /* material of the mesh (KdTree::material)        */
    int32_t kd_root;   /* index of the root in kd_nodes (-1: TRIANGLE)   */
    int32_t tri_base;  /* first triangle of this object in triangles[]   */
    int32_t item_base; /* kd leaf item lists live in kd_items[item_base..] */
    int32_t num_tris;
    int32_t xform;     /* Instance: index into transforms[], else -1     */
    int32_t material_override; /* Instance material (instance.rs:96-98) or -1 */
    double bmin[3], bmax[3]; /* kd boundary in the shape's own space (KdTree::boundary) */
    double origin[3], b0[3], b1[3]; /* Rectangle parameters (rectangle.rs:6-13) */
    double area;       /* Sampleable::area of the shape (own space)      */
    double radius;     /* Sphere radius                                  */
} lumo_object;

typedef struct {
    int32_t v[3];   /* vertex indices into vertices[]                 */
    int32_t n[3];   /* shading-normal indices or -1                   */
    int32_t t[3];   /* uv indices or -1                               */
    int32_t material;
} lumo_triangle;

typedef struct {
    /* geometry */
    int32_t num_vertices, num_normals, num_uvs, num_triangles;
    const double* vertices; /* xyz f64 */
    const double* normals;  /* xyz f64 */
    const double* uvs;      /* uv f64  */
    const lumo_triangle* triangles;
    /* per-object kd-trees */
    int32_t num_kd_nodes, num_kd_items;
    const lumo_kd_node* kd_nodes;
    const int32_t* kd_items;
    /* objects BVH (Scene::objects) */
    int32_t num_objects, num_object_nodes, num_object_items;
    const lumo_object* objects;
    const lumo_bvh_node* object_nodes;
    const int32_t* object_items;
    /* lights BVH (Scene::lights) + power alias table (bvh.rs:105-191) */
    int32_t num_lights, num_light_nodes, num_light_items;
    const lumo_object* lights;
    const lumo_bvh_node* light_nodes;
    const int32_t* light_items;
    const double* alias_prob;  /* alias_table[i].0 */
    const int32_t* alias_idx;  /* alias_table[i].1 */
    const double* alias_pdf;   /* alias_pdf[i]     */
    /* materials and 95-bin dense spectra (dense_spectrum.rs) */
    int32_t num_materials, num_dense_spectra;
    const lumo_material* materials;
    const double* dense_spectra; /* num_dense_spectra x 95 */
    /* instance transforms referenced by lumo_object.xform */
    int32_t num_transforms, pad1;
    const lumo_transform* transforms;
    /* textures (texture.rs), their texels (Spectrum per pixel), bump maps, Perlin lattices */
    int32_t num_textures, num_texels;
    const lumo_texture* textures;
    const lumo_spectrum* texels;
    int32_t num_normal_maps, num_normal_texels;
    const lumo_normal_map* normal_maps;
    const double* normal_texels; /* xyz f64 */
    int32_t num_perlin, pad2;
    const lumo_perlin* perlin;
} lumo_scene_desc;

/* Camera (camera.rs:17-38, CameraConfig): world_to_camera, screen_to_raster and
 * camera_to_screen transforms as (m, inv) row-major 4x4 pairs.  Camera::Perspective or
 * Camera::Orthographic (camera.rs:127-132; generate_ray :257-268).  lumo's orthographic camera
 * has no importance functions (camera.rs:348-351 `unimplemented!()`), so BDPT with it is
 * LUMO_ERR_UNSUPPORTED, as it panics in lumo. */
typedef struct {
    double world_to_camera[2][16];
    double screen_to_raster[2][16];
    double camera_to_screen[2][16];
    double lens_radius, focal_length;
    int64_t width, height;
    int32_t orthographic; /* 0 = Perspective, 1 = Orthographic */
    int32_t illuminant;   /* dense_spectra index used for white balance */
    double white_balance[9];   /* ColorSpace::wb_matrix (space.rs:144-151), row-major */
    double xyz_to_rgb[9];      /* colour space XYZ->RGB (default DCI-P3, space.rs:51-54) */
    double filter_radius, filter_sigma; /* PixelFilter::Gaussian (filter.rs:20-24) */
} lumo_camera_desc;

/* RenderTask (renderer/task.rs:86-104): one tile x one sample batch. */
typedef struct {
    uint64_t px_min[2], px_max[2]; /* tile [px_min, px_max) in raster space */
    uint64_t batch;                /* sample batch index (256 spp per batch) */
    uint64_t samples;              /* samples in this batch                  */
    uint64_t total_samples;        /* Renderer::num_samples                  */
    uint64_t seed;                 /* task seed from the renderer stream     */
} lumo_tile_task;

/* RenderTaskResult (renderer/task.rs:106-116) + its FilmTile pixels (film/tile.rs).
 * `rgb_w` is caller-allocated: 4 doubles (sum w*r, w*g, w*b, sum w) per pixel of the
 * tile, row-major over [px_min, px_max). */
/* A light-tracing splat of BDPT (FilmSample with splat = true): filtered RGB added to the
 * full-frame splat buffer at pixel (x, y) (film/tile.rs:96-101, film.rs:167-170). */
typedef struct {
    uint32_t x, y;
    double rgb[3];
} lumo_splat;

typedef struct {
    double* rgb_w;
    uint64_t num_camera_rays;
    uint64_t num_rays;       /* sum of FilmSample.cost (path depth), task.rs:65 */
    uint64_t num_queries;    /* closest-hit + shadow visibility queries issued  */
    /* BDPT splats of this task in lumo's order; caller-allocated `splat_cap` entries.  On
     * return num_splats is the count produced; a count above splat_cap fails the call with
     * LUMO_ERR_OOM (retry with a larger buffer). */
    lumo_splat* splats;
    uint64_t splat_cap;
    uint64_t num_splats;
} lumo_tile_result;

enum { LUMO_RNG_WAVEFRONT = 0, LUMO_RNG_LUMO_ORDER = 1 };
/* SamplerType (samplers.rs:6-17), the pixel sampler of Renderer::sampler (renderer.rs:89-93).
 * Sobol draws from a 10-bit sequence (samplers/sobol_seq.rs: SOBOL_MAX_LEN 1023): more than 1023
 * samples per pixel panic in lumo and are LUMO_ERR_INVALID here. */
enum { LUMO_SAMPLER_MULTI_JITTERED = 0, LUMO_SAMPLER_UNIFORM = 1, LUMO_SAMPLER_JITTERED = 2, LUMO_SAMPLER_SOBOL = 3 };
enum { LUMO_INTEGRATOR_PATH_TRACE = 0, LUMO_INTEGRATOR_BDPT = 1 };

typedef struct {
    int32_t integrator; /* LUMO_INTEGRATOR_*                              */
    int32_t rng_mode;   /* LUMO_RNG_WAVEFRONT (GPU); lumo-order: oracle only */
    int32_t max_paths;  /* cap on paths in flight (0 = all pixels of the call) */
    int32_t tone_map;   /* LUMO_TONEMAP_* applied per sample before the film (task.rs:73-76)  */
    double tone_arg;    /* ToneMap::Clamp upper bound                                          */
    /* BDPT only.  max_vertices: storage per subpath (0 = 128).  A sample whose subpath is longer
     * is re-run with storage for lumo's maximum depth (1025); more than 4096 such samples in one
     * pass fail the call with LUMO_ERR_UNSUPPORTED (never truncated).  splat_film: optional
     * row-major width x height x 3 array; when a task's result has no `splats` list, its
     * light-tracing taps are summed into it (film.rs:167-170; summation order unspecified, as
     * lumo's tile completion order). */
    int32_t max_vertices;
    int32_t sampler;    /* LUMO_SAMPLER_* (0 = MultiJittered, lumo's default)                  */
    double* splat_film;
} lumo_render_cfg;
enum { LUMO_TONEMAP_NONE = 0, LUMO_TONEMAP_CLAMP = 1, LUMO_TONEMAP_REINHARD = 2 }; /* tone_mapping.rs */

/* Ray batch for traversal-only queries (parity + micro-benchmarks). */
typedef struct {
    const double* origin; /* n x 3 */
    const double* dir;    /* n x 3 */
    const double* t_max;  /* n (closest: ignored, INF) */
    const int32_t* light; /* n: light index for visibility queries (any_hit mode) */
} lumo_ray_soa;

typedef struct {
    double* t;       /* closest: hit t (INF on miss); visibility: light t or INF if occluded */
    int32_t* kind;   /* 0 miss, 1 object, 2 light                                      */
    int32_t* object; /* object / light index                                           */
    int32_t* prim;   /* triangle index (global)                                        */
} lumo_hit_soa;

/* Per-stage device time (HIP events; only with LUMO_OPT_TIMING on), launch
 * counts, query counts and traversal counters (AABB slab tests, kd split-node visits,
 * triangle tests) of the closest-hit [0] and shadow / connection [1] kernels, summed over
 * renders.  BDPT: CLOSEST + SHADE are the subpath walks, RESOLVE the re-runs + fold, BD_* the
 * connection items.  samples_{nan,neg,large} count the camera samples whose radiance has a NaN,
 * a negative or a > 1000 component (the debug_assertions checks of tone_mapping.rs:42-56,
 * counted instead of recoloured; the image is unchanged). */
enum { LUMO_STAGE_CAMERA = 0, LUMO_STAGE_CLOSEST, LUMO_STAGE_SHADE, LUMO_STAGE_SHADOW, LUMO_STAGE_RESOLVE,
       LUMO_STAGE_FINISH, LUMO_STAGE_FILM, LUMO_STAGE_RING, LUMO_STAGE_BD_TRACE_A, LUMO_STAGE_BD_EVAL_A,
       LUMO_STAGE_BD_VIS, LUMO_STAGE_BD_PATHS, LUMO_STAGE_COUNT };
typedef struct {
    double kernel_ms[LUMO_STAGE_COUNT];
    uint64_t launches[LUMO_STAGE_COUNT];
    uint64_t closest_queries, shadow_queries, bounces;
    uint64_t aabb_tests[2], kd_nodes[2], tri_tests[2];
    uint64_t samples_nan, samples_neg, samples_large;
    /* shadow queries (included in shadow_queries) whose contribution is zero whatever the
     * visibility: the record's BSDF pdf is 0, so mis_sample returns 0 before using the hit
     * (integrator.rs:146); the device answers them without traversing the scene. */
    uint64_t shadow_resolved;
    /* closest queries (included in closest_queries) run by the path tracer's tail kernel past
     * the first bounce it takes: > 0 when the device switched a pass to the tail kernel (ABI 9) */
    uint64_t tail_queries;
    /* bounces whose closest-hit rays were sorted before their walks (LUMO_OPT_RAY_SORT; ABI 10) */
    uint64_t sorted_bounces;
} lumo_stats;

/* Per-path dump of one task (test hook for per-path parity): arrays sized samples x pixels
 * (pass-major, pixel raster order within the tile); delta has one entry per pass. */
typedef struct {
    double* radiance;  /* 4 per path */
    double* lambda_;   /* 4 per path */
    double* raster;    /* 2 per path */
    uint64_t* depth;
    double* delta;
} lumo_path_dump;

/* --- context ---------------------------------------------------------------------- */
/* Replaces: ThreadPool::new + RenderTaskExecutor::new (pool.rs:17-38, task.rs:12-21). */
lumo_status lumo_create(int device, void** ctx_out);
void lumo_destroy(void* ctx);
const char* lumo_status_str(lumo_status st);
int lumo_abi_version(void);
/* Number of visible GPUs (0 when the HIP runtime has none). */
int lumo_device_count(void);

/* Replaces: Renderer::new(scene, ...) -> scene.build() + Arc<Scene> (renderer.rs:40-63). */
lumo_status lumo_scene_upload(void* ctx, const lumo_scene_desc* scene);
/* Replaces: Arc<Camera> shared with the executor (task.rs:4-10). */
lumo_status lumo_camera_set(void* ctx, const lumo_camera_desc* camera);

/* Replaces: Executor<RenderTask, RenderTaskResult>::exec (pool.rs:6-8, task.rs:24-82),
 * batched: all n tasks are rendered as one wavefront. */
lumo_status lumo_render_tiles(void* ctx, const lumo_tile_task* tasks, size_t n,
                              const lumo_render_cfg* cfg, lumo_tile_result* out);

/* Replaces: Scene::hit (scene.rs:119-147) when any_hit == 0, and
 * Scene::hit_light (scene.rs:165-189) when any_hit != 0.  Host buffers in and out. */
lumo_status lumo_trace(void* ctx, const lumo_ray_soa* rays, size_t n, lumo_hit_soa* hits,
                       int any_hit);

lumo_status lumo_stats_get(void* ctx, lumo_stats* stats);
lumo_status lumo_stats_reset(void* ctx);
/* Busy time of a set of stages (bit k = LUMO_STAGE k) since the last reset, with timing on: the
 * length of the union of their launches' intervals.  kernel_ms sums launch durations, which counts
 * twice the time that launches on concurrent streams overlap (pipelined passes); this does not. */
lumo_status lumo_stats_busy_ms(void* ctx, uint32_t stage_mask, double* ms);
/* ---------------------------------------------------------------------------------
 * Per-context execution options.  Every option changes only how the work is scheduled on the
 * device, never a result: all values give bit-identical films, counters and traces.  Options are
 * state of the context, so contexts (on one GPU or on several) driven from different host
 * threads do not interfere (lumo's executors share nothing but the task receiver, pool.rs:17-38).
 * A context starts from the defaults below, overridden by the environment variable named beside
 * each (read once, in lumo_create).  Options marked "upload" take effect at the next
 * lumo_scene_upload.  lumo_set_option returns LUMO_ERR_INVALID for an unknown option or a value
 * out of range.
 * ------------------------------------------------------------------------------- */
enum {
    LUMO_OPT_TIMING = 0,       /* per-launch HIP-event timing of every stage: 0 / 1 (LUMO_TIMING, 0)   */
    LUMO_OPT_LDS_STAGING,      /* stage a scene of <= 48 KiB whole in LDS: 0 / 1 (LUMO_LDS, 1)          */
    LUMO_OPT_TOP_STAGING,      /* TOP staging of larger scenes: 0 / 1 (LUMO_TOP, 1)                    */
    LUMO_OPT_FUSED,            /* n_shadow = 1: -1 fused bounce when LDS-staged, 0 three kernels,
                                  1 fused (LUMO_FUSED, -1)                                          */
    LUMO_OPT_TAIL_BELOW,       /* n_shadow = 1: tail kernel below this many live paths, 0 never,
                                  0-2^31 (LUMO_TAIL, 65536)                                        */
    LUMO_OPT_PIPELINE,         /* passes overlapped: 0 off, fused bounces 1-3 head streams, split
                                  schedule on when > 0 (LUMO_PIPELINE, 3)                            */
    LUMO_OPT_HEADS,            /* fused pipeline: bounces per pass on its head stream, 0 auto,
                                  1-64 (LUMO_HEADS, 0)                                              */
    LUMO_OPT_MERGE_PASSES,     /* fused and split pipelines: consecutive passes whose cameras and
                                  head bounces (those before Russian roulette) run as one queue,
                                  0 auto, 1-8 (LUMO_MERGE, 0)                                        */
    LUMO_OPT_DYN_FETCH,        /* fused bounce: blocks fetch paths from a counter: 0 / 1 (LUMO_DYN, 0)*/
    LUMO_OPT_BOUNCE_THREADS,   /* fused bounce: threads per block 64 / 128 / 256
                                  (LUMO_BOUNCE_THREADS, 256)                                        */
    LUMO_OPT_SPLIT_PIPE,       /* split schedule: units in flight 1-4 (LUMO_SPLIT_PIPE, 4)           */
    LUMO_OPT_SPLIT_GROUPS,     /* split schedule: independent task groups 1-4 (LUMO_SPLIT_GROUPS, 2) */
    LUMO_OPT_BDPT_TAIL,        /* BDPT: walk-tail kernel below this many live subpaths, 0 never,
                                  0-2^31 (LUMO_BDPT_TAIL, 65536)                                    */
    LUMO_OPT_BOUNCE_AHEAD,     /* bounces enqueued ahead of the host's count snapshots 1-15 (the
                                  pipelined schedules keep 16 snapshot slots per pass set)
                                  (LUMO_BOUNCE_AHEAD, 3)                                            */
    LUMO_OPT_LDS_GRID,         /* grid cap of LDS-staged kernels, 1-2^20
                                  (LUMO_LDS_GRID, 1.5 x CUs = 384)                                  */
    LUMO_OPT_TOP_GRID,         /* grid cap of TOP kernels, 1-2^20
                                  (LUMO_TOP_GRID, half the CU count = 128)                          */
    LUMO_OPT_TOP_KB,           /* upload: TOP set budget in KiB, 0 to the CU's LDS (160 on MI355X)
                                  (LUMO_TOP_KB, the CU's LDS)                                       */
    LUMO_OPT_KD_LDS,           /* upload: kd stack entries per thread in LDS in TOP kernels, 0-64
                                  (LUMO_KD_LDS, 8)                                                  */
    LUMO_OPT_STACK_CLASS,      /* upload: kd stack class override, 0 auto or one of 4 / 8 / 16 / 24 /
                                  32 / 48 / 64; never below the scene's need (LUMO_STACK_CLASS, 0)  */
    LUMO_OPT_FULL_KERNELS,     /* upload: general feature kernels even for lean scenes: 0 / 1
                                  (LUMO_FULL_KERNELS, 0)                                            */
    LUMO_OPT_POISON,           /* debug: fill every newly allocated device buffer with 0xFF bytes,
                                  so a read of a buffer before its first write shows: 0 / 1
                                  (LUMO_POISON, 0)                                                  */
    LUMO_OPT_TAIL_PRIORITY,    /* fused pipeline: the stream of the passes' tails, films and rings (the
                                  chain each pass's Russian roulette waits on) at high priority: 0 / 1
                                  (LUMO_TAIL_PRIORITY, 0)                                           */
    LUMO_OPT_TOP_KD,           /* upload: the TOP set's spare LDS holds the top treelets of the
                                  largest kd tree: 0 / 1 (LUMO_TOP_KD, 1)                           */
    LUMO_OPT_TAIL_BOUNCES,     /* fused pipeline: fused bounces per pass the tail stream runs before the
                                  tail kernel, -1 auto (2 for one-pass units, 0 for merged ones), 0-16
                                  (LUMO_TAIL_BOUNCES, -1)                                           */
    LUMO_OPT_FILM_FIRST,       /* fused pipeline, film on the tail stream: the unit's film before its
                                  last ring: 0 / 1 (LUMO_FILM_FIRST, 0)                             */
    LUMO_OPT_BDPT_TOP,         /* BDPT connection visibility (k_bdpt_vis) of scenes too large to stage
                                  whole reads the TOP set and kd stack columns from LDS: 0 / 1
                                  (LUMO_BDPT_TOP, 1)                                                */
    LUMO_OPT_BDPT_GROUPS,      /* BDPT: task groups rendered as concurrent chains of passes on their own
                                  streams, 1-4 (LUMO_BDPT_GROUPS, 2; ABI 9)                          */
    LUMO_OPT_RAY_SORT,         /* three-kernel bounces: the closest-hit rays of a bounce radix-sorted
                                  before their walks: 0 off, 1 direction octant major, 2 origin cell
                                  major, -1 auto (1 for kd stack class >= 32) (LUMO_RAY_SORT, -1; ABI 9)*/
    LUMO_OPT_ACCEL,            /* upload: acceleration structure the walks use.  0 lumo's own (the
                                  objects / lights BVHs, bvh.rs, and per-mesh kd-trees, kdtree.rs;
                                  bit-exact with the reference), 1 wide (a 4-wide SAH BVH over all
                                  primitives, nearest child first; same hit semantics except ties and
                                  BDPT's visible()) (LUMO_ACCEL, 0; ABI 10)            */
    LUMO_OPT_COUNT
};
lumo_status lumo_set_option(void* ctx, int32_t option, int64_t value);
lumo_status lumo_get_option(void* ctx, int32_t option, int64_t* value);

/* The schedule the last lumo_render_tiles call used (after its last max_paths chunk): which
 * pass loop ran and with how many streams, units, groups and merged passes.  Lets callers and
 * tests check that a requested schedule was not cut back (free HBM bounds the split schedule's
 * units in flight). */
enum { LUMO_SCHED_SEQUENTIAL = 0, LUMO_SCHED_FUSED_PIPELINE = 1, LUMO_SCHED_SPLIT_PIPELINE = 2,
       LUMO_SCHED_BDPT_GROUPS = 3 /* ABI 9 */ };
typedef struct {
    int32_t schedule;        /* LUMO_SCHED_*                                               */
    int32_t head_streams;    /* fused pipeline: head streams                               */
    int32_t head_bounces;    /* fused pipeline: bounces per pass on the head stream        */
    int32_t merged_passes;   /* fused / split pipeline: passes per head unit               */
    int32_t units_in_flight; /* split pipeline: (group, pass) units in flight; BDPT groups  */
    int32_t task_groups;     /* split pipeline / BDPT groups: independent task groups      */
    int32_t fused;           /* 1: fused bounce kernel, 0: three kernels per bounce         */
    int32_t tail_bounces;    /* fused pipeline: fused bounces per pass on the tail stream   */
} lumo_schedule_info;
lumo_status lumo_last_schedule(void* ctx, lumo_schedule_info* info);

/* Test hook: render one task in the wavefront order and dump every path. */
lumo_status lumo_debug_paths(void* ctx, const lumo_tile_task* task, lumo_path_dump* dump);
/* Integrator of lumo_debug_paths (LUMO_INTEGRATOR_*; BDPT splats are not collected there). */
lumo_status lumo_debug_set_integrator(void* ctx, int integrator);
/* Pixel sampler of lumo_debug_paths (LUMO_SAMPLER_*). */
lumo_status lumo_debug_set_sampler(void* ctx, int sampler);
/* Diagnostics: per-bounce record (20 doubles per bounce, at most 64 bounces) of the path of
 * `pixel` in sample pass `pass` of `task`; *n_out = number of bounces recorded. */
lumo_status lumo_debug_trace(void* ctx, const lumo_tile_task* task, int pass, int pixel, double* out,
                             int* n_out);
/* Kernel variant selected for the uploaded scene: kd stack class, bytes of scene staged in LDS
 * (0: no staging), feature class (1: instances / spheres / triangle lights / microfacet
 * materials), shadow rays per bounce (scene.rs:90-92).  Scenes too large to stage whole stage
 * their TOP set in the closest-hit and visibility kernels: top_bytes of LDS per block (0: none),
 * holding the first top_object_nodes / top_light_nodes nodes (breadth-first: the top levels) of
 * the objects / lights BVH, the object items and the objects' traversal records. */
typedef struct {
    int32_t stack_class, lds_bytes, full_kernels, n_shadow;
    int32_t top_bytes, top_object_nodes, top_light_nodes;
    int32_t top_kd_nodes; /* kd nodes of the largest kd tree (its top treelets) in the TOP set */
    int32_t top_shm;      /* LDS per TOP block: the TOP set + the kd stack columns, within
                             LUMO_OPT_TOP_KB (ABI 9)                                          */
    /* ABI 10: the acceleration structure the uploaded scene is walked with (LUMO_OPT_ACCEL: 0 lumo,
     * 1 wide; 0 also when wide was asked for and the build refused the scene, e.g. a tree needing
     * more than 64 walk stack entries) and, for wide, its nodes, leaf triangle records, deepest
     * walk stack, node levels and the nodes of its TOP set (a breadth-first prefix) */
    int32_t accel, wide_nodes, wide_tris, wide_stack, wide_depth, top_wide_nodes;
} lumo_scene_info_t;
lumo_status lumo_scene_info(void* ctx, lumo_scene_info_t* info);
/* Diagnostics: one coalesced 8-B-per-lane read stream and one write stream over n doubles
 * (kernels k_calib_read8 / k_calib_write8), to calibrate rocprofv3 FETCH_SIZE / WRITE_SIZE for
 * the access width of the path kernels. */
lumo_status lumo_debug_stream(void* ctx, size_t n);
/* Diagnostics (ABI 10): the device's exclusive prefix sum (device/scan.h, the BDPT item lists' scan)
 * of n host uint32 counts into out (n = 0: nothing is written). */
lumo_status lumo_debug_scan(void* ctx, const uint32_t* in, uint32_t* out, size_t n);

/* ---------------------------------------------------------------------------------
 * Feature buffers: the first hit's albedo, shading normal and depth of every film sample, for
 * denoisers and compositing.  An addition within ABI 10: no existing layout changes, so the
 * capability check is the presence of these two symbols (dlsym), not the version.
 *
 * A feature render takes the same tasks, sampler and seeds as lumo_render_tiles and is aligned
 * with its film sample for sample: sample (task, pass, pixel) has the beauty sample's raster
 * position, lens point and wavelengths, lands in the planes with the beauty film's filter weights
 * summed in the same order, and channel 3 of every plane is the beauty tile's sum w bit for bit.
 * The camera ray's Scene::hit (scene.rs:119-147) gives the record; nothing is followed through
 * mirrors or glass.  Per sample:
 *   kind, object, prim   as lumo_trace: 0 miss, 1 object, 2 light; index; global triangle or -1
 *   material, backface   the hit's material index (-1 on a miss), Hit::backface (hit.rs:37-59)
 *   t, p, ng, uv         the hit record (uv wrapped; the ray is normalised, so t is a distance)
 *   ns                   the shading normal with the bump map applied (material.rs:323-331)
 *   n                    backface ? -ns : ns (the normal feature)
 *   albedo               at the sample's 4 wavelengths: kd of Lambertian / MfDiffuse, ks of
 *                        MfConductor, tf of MfDielectric, 1 for a light, 0 for Blank
 *   albedo_rgb           albedo through the film's spectrum -> XYZ -> white balance -> RGB,
 *                        without a tone map
 * All are 0 on a miss (material -1, object and prim -1).
 * ------------------------------------------------------------------------------- */
/* Filtered planes of one task: caller-allocated, 4 doubles per tile pixel laid out as rgb_w; a
 * NULL plane is skipped.  A miss contributes its weight with zero features.
 *   albedo_w   sum w albedo_rgb, sum w
 *   normal_w   sum w n, sum w
 *   depth_w    sum w t hit, sum w hit, 0, sum w   (hit = 1 when kind != 0): depth is channel 0
 *              over channel 1, coverage channel 1 over channel 3 */
typedef struct {
    double* albedo_w;
    double* normal_w;
    double* depth_w;
} lumo_feature_planes;
typedef struct {
    int32_t sampler;   /* LUMO_SAMPLER_* */
    int32_t max_paths; /* cap on paths in flight (0 = all pixels of the call), as lumo_render_cfg */
} lumo_feature_cfg;
/* Per-sample records of one task: arrays sized samples x pixels, pass-major, pixels in raster
 * order within the tile (as lumo_path_dump); the number after each name is its doubles / ints per
 * sample.  A NULL array is skipped. */
typedef struct {
    int32_t* kind;       /* 1 */
    int32_t* object;     /* 1 */
    int32_t* prim;       /* 1 */
    int32_t* material;   /* 1 */
    int32_t* backface;   /* 1 */
    double* t;           /* 1 */
    double* p;           /* 3 */
    double* ng;          /* 3 */
    double* ns;          /* 3 */
    double* n;           /* 3 */
    double* uv;          /* 2 */
    double* albedo;      /* 4 */
    double* albedo_rgb;  /* 3 */
    double* raster;      /* 2 */
    double* lambda_;     /* 4 */
} lumo_feature_dump;
/* The feature planes of n tasks (cfg NULL: MultiJittered, no cap), chunked by max_paths as
 * lumo_render_tiles.  Serves both integrators (the camera path is the same).  Errors as
 * lumo_render_tiles: LUMO_ERR_INVALID (NULL context, tasks or out, a malformed task, an unknown
 * sampler, Sobol with more than 1023 samples), LUMO_ERR_NO_SCENE, LUMO_ERR_NO_CAMERA.  Leaves
 * lumo_last_schedule's record as it is. */
lumo_status lumo_render_features(void* ctx, const lumo_tile_task* tasks, size_t n, const lumo_feature_cfg* cfg,
                                 lumo_feature_planes* out);
/* Test hook: the per-sample records of one task, with the sampler of lumo_debug_set_sampler. */
lumo_status lumo_debug_features(void* ctx, const lumo_tile_task* task, lumo_feature_dump* dump);

/* ---------------------------------------------------------------------------------
 * Denoiser: an edge-avoiding a-trous wavelet filter guided by the feature planes, with albedo
 * demodulation and a spatial variance estimate (the spatial part of SVGF; lumo_denoise_temporal
 * below is the temporal part).  An addition within ABI 10: the capability check is the presence
 * of lumo_denoise (dlsym).
 *
 * Inputs and outputs are host arrays of a whole frame, height x width, row-major: the film's
 * rgb_w and the three feature planes as lumo_render_tiles / lumo_render_features produce them
 * (4 doubles per pixel), and optionally add_rgb (3 per pixel), added to the colour after the
 * division by sum w (BDPT: splat_scale * splats / filter integral).  All arithmetic is f64 in the
 * order below, never contracted; exp is lm_exp (common/lmath.h); max(x, f) is x > f ? x : f and
 * min(x, f) is x < f ? x : f; a sum starts at 0.0 and adds its taps in row-major order (dy outer,
 * dx inner, ascending); a tap outside the image is skipped unless a step says clamped.
 *   1 prepare   c = rgb_w[0..2] / rgb_w[3] (0 when rgb_w[3] = 0), + add_rgb;
 *               cov = depth_w[1] / depth_w[3], z = depth_w[0] / depth_w[1] (each 0 when its
 *               denominator is 0); hit = cov > 0; n = normal_w[0..2] / sqrt((x x + y y) + z z) (0
 *               when that is 0); a = albedo_w[0..2] / albedo_w[3] (0 when albedo_w[3] = 0);
 *               a' = max(a + (1 - cov), albedo_floor) when demodulate, else 1; e = c / a';
 *               l = (0.2126 e0 + 0.7152 e1) + 0.0722 e2;
 *               fz = max(|z(x+1, y) - z|, |z(x, y+1) - z|), coordinates clamped
 *   1b firefly  only when lumo_denoise_set_firefly (below, with the step's definition) has set it:
 *               e and l of a hit pixel that stands out from its alike neighbours are scaled down
 *   2 pair     centre p, tap q at pixel offset (ox, oy): neither a hit: wn = 1, dz = 0; exactly
 *               one a hit: the tap's weight is 0; else d = max((nx nx' + ny ny') + nz nz', 0),
 *               wn = d squared k times, dz = |z_p - z_q| / ((sigma_z fz_p) sqrt(ox ox + oy oy) +
 *               depth_floor z_p)
 *   3 variance  the (2r+1)^2 window at unit stride, the centre with weight 1, the others with
 *               w = wn exp(-min(dz, 700)): m1 = sum(w l) / sum w, m2 = sum(w (l l)) / sum w,
 *               var = max(m2 - m1 m1, 0)
 *   4 a-trous   iteration i = 0 .. N-1, step s = 2^i: gv = the 3 x 3 binomial (1/4 1/2 1/4 per
 *               axis) of var at unit stride, clamped; taps at (s dx, s dy), dx, dy in -2 .. 2,
 *               h = b[dy+2] b[dx+2], b = (1/16, 1/4, 3/8, 1/4, 1/16); the centre's weight is h, the
 *               others' w = (h wn) exp(-min(dz + dl, 700)), dl = |l_p - l_q| / (sigma_l sqrt(gv) +
 *               lum_floor); e' = sum(w e) / sum w, var' = sum((w w) var) / (sum w sum w); l from e'
 *   5 finish    rgb_out = e a'; variance_out = var
 * Non-finite inputs give unspecified values around them.  The guides are the first hit's, so a
 * reflection or refraction is filtered with the guides of the surface it is seen in.
 * ------------------------------------------------------------------------------- */
typedef struct {
    int64_t width, height;
    const double* rgb_w;    /* 4 per pixel: sum w rgb, sum w */
    const double* albedo_w; /* lumo_feature_planes, assembled into the frame */
    const double* normal_w;
    const double* depth_w;
    const double* add_rgb;  /* 3 per pixel, or NULL */
} lumo_denoise_in;
typedef struct {
    int32_t iterations;        /* N: 1 .. 5 (default 5) */
    int32_t normal_log2_power; /* k: 0 .. 10 (default 7: the normals' dot product to the 128th) */
    int32_t variance_radius;   /* r: 1 .. 3 (default 3) */
    int32_t demodulate;        /* 0 / 1 (default 1) */
    double sigma_l;            /* default 4.0 */
    double sigma_z;            /* default 1.0 */
    double albedo_floor;       /* default 1e-3 */
    double depth_floor;        /* default 1e-3 */
    double lum_floor;          /* default 1e-8 */
    double* stage_ms;          /* NULL, or N + 5 doubles: the call's device times in ms (HIP events) of the
                                  upload, prepare, variance, each a-trous iteration, finish, the read-back */
} lumo_denoise_cfg;
/* lumo_denoise(void* ctx, const lumo_denoise_in* in, const lumo_denoise_cfg* cfg, double* rgb_out,
 * double* variance_out): the denoised linear RGB frame into rgb_out (3 doubles per pixel) and, when
 * variance_out is not NULL, the filtered variance of the demodulated luminance (1 per pixel).  cfg
 * NULL: the defaults.  LUMO_ERR_INVALID for a NULL context, in or rgb_out, a NULL plane among the
 * four, a width or height below 1 (or above 2^20), a cfg field outside its range or a non-finite
 * one; LUMO_ERR_OOM as elsewhere.  Needs no scene or camera; runs on the main stream, returns after
 * the read-back and leaves the stats and lumo_last_schedule's record alone. */
lumo_status lumo_denoise(void* ctx, const lumo_denoise_in* in, const lumo_denoise_cfg* cfg, double* rgb_out,
                         double* variance_out);

/* ---------------------------------------------------------------------------------
 * Temporal denoiser: the other half of SVGF.  The previous call's colour and luminance moments
 * are reprojected through the depth and normal guides and accumulated per pixel, the accumulated
 * moments give the variance that drives the a-trous edge stops where the history is long enough,
 * and one a-trous iteration's output is fed back as the next call's colour history.  An addition
 * within ABI 10: the capability check is the presence of lumo_denoise_temporal (dlsym).
 *
 * The context keeps the history of its last lumo_denoise_temporal call on the device: per pixel
 * the colour history e (3), the luminance moments m1, m2, the history length (an integer), the
 * guides n (3), z and hit, and with them that call's camera.  lumo_denoise_reset drops it, and so
 * does a call with another width or height; lumo_destroy frees it.  A call without history is a
 * first frame and equals lumo_denoise of the same input bit for bit.  lumo_denoise neither reads
 * nor writes the history.
 *
 * The rules are lumo_denoise's: f64, never contracted, exp = lm_exp, max(x, f) = x > f ? x : f,
 * min likewise, sums from 0.0 in row-major order.  xf(T, p) is the point transform of T's matrix
 * (row r: ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 w, then the division by w unless w = 0), xf_inv that
 * of its inverse, with w = 1 for a point and 0 for a direction; normalize(a) = a / sqrt(max((ax ax +
 * ay ay) + az az, 0)) (common/vec.h).  Primed names belong to the previous call.
 *   1 prepare     step 1 of lumo_denoise: e, l, n, z, hit, a', fz; then its step 1b when set
 *   2 position   a hit pixel (x, y): the camera ray of raster point (x + 0.5, y + 0.5) with lens
 *                 radius 0, as k_camera computes it: s = xf_inv(screen_to_raster, (x + 0.5, y + 0.5,
 *                 0)), c = xf_inv(camera_to_screen, s), o = xf_inv(world_to_camera, (0, 0, 0)),
 *                 d = normalize(xf_inv(world_to_camera, normalize(c)) as a direction);
 *                 P = o + z d per component.  A pixel that is not a hit has no history.
 *   3 previous    c' = xf(world_to_camera', P); no history unless c'.z > 0 (the view axis is +z in
 *     raster      camera space); q = xf(screen_to_raster', xf(camera_to_screen', c')); no history
 *                 unless qx and qy are finite; o' = xf_inv(world_to_camera', (0, 0, 0)),
 *                 z' = sqrt(max(|P - o'|^2, 0)) with the squared length summed as in normalize
 *   4 taps        u = qx - 0.5, v = qy - 0.5, x0 = floor(u), y0 = floor(v), fx = u - x0, fy = v - y0
 *                 (a q more than 2 pixels outside the image has no tap inside it: no history).
 *                 Taps (x0 + i, y0 + j), i, j in 0 .. 1, i inner, with w = ((1 - fx) | fx) ((1 - fy)
 *                 | fy).  A tap is valid when it lies inside the image, was a hit, (nx nx' + ny ny')
 *                 + nz nz' >= normal_cos_min and |z_tap - z'| <= depth_rel_max z'.  Over the valid
 *                 taps, sum w > 0: the history of e0, e1, e2, m1, m2 is sum(w h) / sum w and the
 *                 history length the largest valid tap's.  Else the 3 x 3 taps around (floor(u +
 *                 0.5), floor(v + 0.5)), w = 1 each, the same test; none valid: no history.
 *   5 accumulate  with history: N = min(len + 1, max_history), al = max(alpha, 1 / N),
 *                 x_acc = (1 - al) x_hist + al x for e0..2, for m1 from l and for m2 from l l;
 *                 without: N = 1, e_acc = e, m1 = l, m2 = l l
 *   6 variance    N >= min_history: var = max(m2 - m1 m1, 0); elsewhere step 3 of lumo_denoise
 *                 with l the luminance of e_acc
 *   7 a-trous     steps 4 and 5 of lumo_denoise on e_acc and var.  The e' of iteration
 *                 feedback - 1 (e_acc when feedback = 0) becomes the colour history; m1, m2, N, n,
 *                 z, hit and the camera are stored with it.
 * The guides are the first hit's (as lumo_denoise), a miss keeps no history, and a thin lens is
 * treated as a pinhole: the depth of a lens sample is a distance from its lens point, so P is
 * approximate there.
 * ------------------------------------------------------------------------------- */
typedef struct {
    double alpha;           /* 0 .. 1 (default 0.2): blend floor for colour and moments */
    double normal_cos_min;  /* -1 .. 1 (default 0.9): a history tap's normal agrees to this cosine */
    double depth_rel_max;   /* 0 .. 1e6 (default 0.1): a history tap's depth agrees to this fraction */
    int32_t max_history;    /* 1 .. 1024 (default 32): cap on the history length */
    int32_t min_history;    /* 1 .. 1025 (default 4): history length from which the temporal variance is used */
    int32_t feedback;       /* 0 .. cfg's iterations (default 1): the a-trous iteration whose output becomes
                               the colour history; 0: the unfiltered accumulated colour */
    int32_t stage_lds;      /* 0 / 1 (default 1): 0 forces the direct-gather form of k_dn_reproject; no
                               result depends on it */
} lumo_temporal_cfg;
typedef struct {
    int64_t with_history;    /* pixels whose reprojection found history */
    int64_t without_history; /* the others: width x height - with_history */
    int64_t blocks_staged;   /* k_dn_reproject blocks that tapped the history from their LDS tile */
    int64_t blocks_direct;   /* blocks that tapped it from global memory; a block none of whose pixels has a
                                tap to read (a first frame, a camera turned away) is in neither count */
    double* stage_ms;        /* NULL, or N + 8 doubles: the call's device times in ms (HIP events) in launch
                                order: upload, prepare, reproject, variance, the variance choice, the N
                                iterations with the history write in its place (first when feedback = 0,
                                else after iteration feedback - 1), finish, the read-back.  Set it before
                                the call; cfg's stage_ms is not used */
} lumo_temporal_info;
/* lumo_denoise_temporal: lumo_denoise's arguments, the frame's camera, tcfg (NULL: the defaults) and
 * info (NULL, or filled in).  Errors as lumo_denoise, and LUMO_ERR_INVALID for a NULL camera, a camera
 * whose width or height differs from in's, a tcfg field outside its range or a non-finite one;
 * LUMO_ERR_UNSUPPORTED for an orthographic camera (its depth is not a distance from one point).  A
 * call that fails leaves no history.  A steady-state call uploads what lumo_denoise uploads. */
lumo_status lumo_denoise_temporal(void* ctx, const lumo_denoise_in* in, const lumo_camera_desc* camera,
                                  const lumo_denoise_cfg* cfg, const lumo_temporal_cfg* tcfg, double* rgb_out,
                                  double* variance_out, lumo_temporal_info* info);
/* Drops the context's history: the next lumo_denoise_temporal call is a first frame. */
lumo_status lumo_denoise_reset(void* ctx);

/* ---------------------------------------------------------------------------------
 * Firefly clamp: step 1b of lumo_denoise and of lumo_denoise_temporal.  A hit pixel whose
 * demodulated luminance exceeds an order statistic of its like-guided neighbours' is scaled down
 * to it, before the variance, the a-trous and, in the temporal call, the reprojection and the
 * accumulation see it.  Off unless lumo_denoise_set_firefly has set it: per-context state, as an
 * execution option is, read by both entry points; a first temporal frame equals lumo_denoise under
 * one and the same setting.  An addition within ABI 10: the capability check is the presence of
 * lumo_denoise_set_firefly (dlsym).
 *
 * The rules are lumo_denoise's (f64, never contracted, max(x, f) = x > f ? x : f, min likewise).
 * The step uses step 1's values of all pixels, never a value it has itself changed.  c is step 1's
 * colour before the demodulation (rgb_w[k] / rgb_w[3], 0 when rgb_w[3] = 0, + add_rgb), a' its
 * divisor, e, l, n, z and hit its outputs.
 *   1b firefly   a pixel p that is not a hit is unchanged.  The alike neighbours of a hit p are the
 *                pixels q != p of the (2R+1)^2 window at unit stride that lie inside the image, are
 *                hits, and have (nx nx' + ny ny') + nz nz' >= normal_cos_min and |z_q - z_p| <=
 *                depth_rel_max z_p.  m is their count; m < min_alike: unchanged.  Else v is the
 *                rank-th largest l_q among them (ties are values), b = gain v, and when l_p > b:
 *                g = b / l_p, c'_k = c_k g, e_k = c'_k / a'_k, l = (0.2126 e0 + 0.7152 e1) + 0.0722 e2.
 *                Else (a NaN l_p among it) unchanged.
 * So the step equals the unchanged definition on a frame whose rgb_w is (c', 1) with no add_rgb.
 * A miss is never clamped (a small sun seen directly survives); a directly seen emitter of fewer
 * than rank + 1 pixels on a surface is.  With the clamp on, the `prepare` interval of stage_ms
 * includes the step.
 * ------------------------------------------------------------------------------- */
typedef struct {
    int32_t radius;         /* R: 1 .. 3 (default 2) */
    int32_t rank;           /* 1 .. 8 (default 2) */
    int32_t min_alike;      /* rank .. 48 (default 4) */
    int32_t reserved;       /* 0 */
    double gain;            /* 1 .. 1e6 (default 1.0) */
    double normal_cos_min;  /* -1 .. 1 (default 0.9) */
    double depth_rel_max;   /* 0 .. 1e6 (default 0.1) */
} lumo_firefly_cfg;
typedef struct {
    int64_t clamped; /* pixels the step changed in the context's last denoise call; 0 when off */
    double ms;       /* the step's device time in that call (HIP events); 0 when off */
} lumo_firefly_info;
/* cfg NULL: off, the state of a new context.  LUMO_ERR_INVALID for a NULL context, a field outside
 * its range, a non-finite one or min_alike < rank; the setting is then as it was. */
lumo_status lumo_denoise_set_firefly(void* ctx, const lumo_firefly_cfg* cfg);
/* Of the context's last lumo_denoise / lumo_denoise_temporal call whose arguments were valid (zeros
 * before the first, when the clamp was off, and when that call then failed). */
lumo_status lumo_denoise_firefly_info(void* ctx, lumo_firefly_info* info);

/* ---------------------------------------------------------------------------------
 * Device builder of the wide BVH (LUMO_OPT_ACCEL = 1).  By default the upload builds the 4-wide BVH
 * on the host (binned SAH, seconds for a large scene).  lumo_scene_set_wide_build lets a context
 * build it on the GPU instead, as an LBVH, in milliseconds: for scenes whose geometry changes from
 * frame to frame.  Same node format, same arrays, same walks; the tree differs, so the traversal
 * counters do, and a ray that ties between two triangles of one tree may keep the other one.
 * Per-context state read by the next lumo_scene_upload, as the firefly clamp's; an addition within
 * ABI 10, the capability check is the presence of lumo_scene_set_wide_build (dlsym).
 *
 * The construction, step by step (f64 throughout; deterministic: no float atomics, positions from
 * scans, the one atomic counter per node only decides which thread carries on):
 *   0 host      per tree (world objects, world lights, one BLAS per distinct (tri_base, count)): its
 *               runs of triangles and its object leaves (a sphere, an instance) with their world
 *               boxes by the host builder's rules.  The refusal of light kd trees deeper than 16
 *               levels stays here.
 *   1 boxes     per primitive the exact f64 min / max of its vertices; centroid 0.5 lo + 0.5 hi;
 *               per tree the bounds of the centroids.
 *   2 keys      63-bit Morton key, 21 bits per axis (x most significant): cell =
 *               (c - lo) / (hi - lo) 2^21 truncated, at most 2^21 - 1; a zero extent or a NaN: cell 0.
 *   3 sort      stable LSD radix sort of (tree, key), 8-bit digits, starting from primitive order:
 *               equal keys stay in primitive order.
 *   4 tree      Karras's binary radix tree per tree; delta(i, j) = clz(key_i ^ key_j), and
 *               64 + clz(i ^ j) (32-bit positions) when the keys are equal.
 *   5 fit       bottom-up: box = union of the children's, primitive count, "holds an object leaf".
 *               A subtree of at most leaf_max primitives, none an object leaf, is a leaf when its
 *               parent is none; an object leaf is a leaf of its own (count 0).  Leaf records are
 *               the triangles in sorted order.
 *   6 collapse  level by level from every tree's root (objects, lights, BLASes): a node's children
 *               are its two binary children, then, while fewer than 4, the largest-half-area child
 *               that is no leaf replaced in place by its two (the first such on ties).  Node
 *               indices are level-major, children in item order.  Boxes narrow to f32 outward:
 *               cast, compare back in f64, one ulp by nextafter.  Unused slots: lo 1, hi -1, ref NONE.
 *   7 derived   levels; max |coordinate|; walk-stack need n - 1 + the largest child need, an
 *               instance leaf 1 + the deepest BLAS need; refused above stack_limit or at 2^27 leaf
 *               records.  sah_cost (both builders): over the trees whose root is a node, the sum
 *               over nodes and children of child half-area / half-area of the union of the root's
 *               child boxes, times the triangle count of a leaf (1 for a node or an object leaf).
 * Asked for the device builder and refused: the host builder; that refused too: lumo's structures.
 * ------------------------------------------------------------------------------- */
typedef struct {
    int32_t builder;     /* 0 host SAH (default), 1 device LBVH; read at the next upload with accel = 1 */
    int32_t leaf_max;    /* 1 .. 8 (default 8): triangles per leaf of the device builder */
    int32_t stack_limit; /* 1 .. 64 (default 64): the device build is refused above this walk-stack need */
    int32_t reserved;    /* 0 */
} lumo_wide_build_cfg;
/* cfg NULL: the defaults.  LUMO_ERR_INVALID for a NULL context or a field outside its range; the
 * setting is then as it was. */
lumo_status lumo_scene_set_wide_build(void* ctx, const lumo_wide_build_cfg* cfg);

typedef struct {
    int32_t builder_asked, builder_used;   /* used: -1 when the scene is walked on lumo's structures */
    int32_t trees;     /* trees with a primitive (world objects, world lights, BLASes) */
    int32_t levels;    /* node levels (lumo_scene_info's wide_depth + 1; 0: no node) */
    int32_t nodes, tris, stack, reserved;
    double build_ms;   /* device builder: HIP events around steps 1-7; host builder: wall clock of its build */
    double sah_cost;
} lumo_wide_build_info;
/* Of the last upload (zeros with builder_used -1 when accel = 0).  LUMO_ERR_NO_SCENE before one. */
lumo_status lumo_scene_wide_build_info(void* ctx, lumo_wide_build_info* info);

/* ---------------------------------------------------------------------------------
 * Clustered device builder.  The LBVH above splits where the Morton keys say; its SAH cost is 1.3 to
 * 2.2 times the host tree's.  lumo_scene_set_wide_cluster has the device builder make its binary tree
 * bottom-up by surface area instead: parallel locally-ordered clustering (PLOC, Meister & Bittner
 * 2018).  A second per-context setting, read by the next upload with accel = 1 when the device
 * builder is used and inert otherwise; an addition within ABI 10, found by dlsym like the above.
 * Steps 0 to 3 and 6 to 7 above stay; in place of 4 and 5 (f64, no atomic, positions from scans):
 *   4' clusters  one cluster per sorted primitive: its ref, tree and box, a compact array in Morton
 *               order.  A tree's clusters are contiguous and stay so.
 *   5' iterate   until every tree is one cluster.  (a) Each cluster i finds its nearest neighbour
 *               among the clusters j of its tree with 0 < |i - j| <= radius: the smallest half-area
 *               of the union box (min / max, then dx dy + dy dz + dz dx; a negative or NaN extent: 0;
 *               a NaN area: +inf), the smaller j on ties.  (b) Every pair that chose each other
 *               becomes one internal node: children (i, j) for i < j, box the union, primitive
 *               count, "holds an object leaf"; it takes i's place and j leaves, the others keep
 *               their order.  A tree of `live` clusters gives the merges of an iteration the slots
 *               base + live - 2 downward in cluster order, so its root is slot base.  Every tree of
 *               two or more clusters merges at least one pair per iteration.  After max_iter
 *               iterations (a) is replaced by pairing clusters 2k and 2k + 1 of each tree, which
 *               halves every tree: nested boxes can merge one pair per iteration.
 *   5'' relabel a leaf's position within its tree becomes the number of primitives to its left in
 *               the binary tree, so every subtree is a range of positions again; leaf records are
 *               the triangles in that order, and a leaf is chosen as in 5.
 * ------------------------------------------------------------------------------- */
typedef struct {
    int32_t radius;    /* 0 (default): the LBVH, exactly as above.  1 .. 64: PLOC with this search radius */
    int32_t max_iter;  /* 0: the built-in cap.  1 .. 4096: nearest-neighbour iterations before
                          the builder switches to pairing adjacent clusters */
    int32_t reserved[2];  /* 0 */
} lumo_wide_cluster_cfg;
/* cfg NULL: the defaults.  LUMO_ERR_INVALID for a NULL context, a field outside its range or a
 * non-zero reserved; the setting is then as it was. */
lumo_status lumo_scene_set_wide_cluster(void* ctx, const lumo_wide_cluster_cfg* cfg);

typedef struct {
    int32_t radius_used;        /* 0 whenever the LBVH, the host tree or lumo's structures were used */
    int32_t iterations;         /* nearest-neighbour iterations */
    int32_t paired_iterations;  /* iterations that paired adjacent clusters */
    int32_t reserved;
    double cluster_ms;          /* HIP events around steps 4' to 5''; lumo_wide_build_info.build_ms holds them too */
} lumo_wide_cluster_info;
/* Of the last upload.  LUMO_ERR_NO_SCENE before one. */
lumo_status lumo_scene_wide_cluster_info(void* ctx, lumo_wide_cluster_info* info);

/* ---------------------------------------------------------------------------------
 * Treelet restructuring of the clustered tree (after Karras & Aila 2013, section 3).  A third
 * per-context setting, read by the next upload; it acts only when the device builder ran with a
 * cluster radius >= 1 and is inert otherwise (the LBVH, the host builder, a refused device build,
 * accel = 0: passes_used, the counts and the areas are then 0).  An addition within ABI 10, found by
 * dlsym.  Between 5' and 5'' (f64; every choice determined; the only atomics are integer counters):
 *   5t treelets  The objective is the sum of the half-area of the box over the internal binary nodes
 *               (half-area as in 5'; a NaN area counts as +inf here throughout); a primitive or an
 *               object leaf costs nothing.  `passes` passes run, each bottom-up: a node is handled
 *               when both of its child subtrees are finished, and the treelets of unrelated nodes
 *               are disjoint subtrees, so the result does not depend on timing.  gamma is the same
 *               in every pass.  At a node R whose subtree holds gamma primitives or more:
 *               (a) Treelet.  Its leaves are R's two children; while fewer than 7, the leaf of
 *               largest half-area that is an internal node is replaced in place by its two children
 *               (the first in treelet order on ties).  Fewer than 7 leaves in the end: R is skipped.
 *               (b) Optimal topology.  For each of the 127 non-empty subsets S of the 7 leaves a(S)
 *               is the half-area of the union box, formed in ascending leaf order; c(S) = 0 for a
 *               single leaf, else c(S) = a(S) + min over the proper non-empty P in S that hold the
 *               lowest leaf of S of (c(P) + c(S \ P)), the numerically smallest P on ties.
 *               (c) Replace only if c(all) is strictly below the cost of the present topology,
 *               summed the same way (a(S) + (cost of one child + cost of the other) at each of its 6
 *               internal nodes, S the node's leaves): the present topology is one of the candidates
 *               of (b), so an equal cost never replaces.  The new internal nodes are the sets of the
 *               optimal topology in pre-order (a node, then its part P, then S \ P); they take the
 *               6 old slots in the order R, then the others as (a) opened them, so R keeps its slot
 *               and a tree's root stays at its base.  Each node's children are (P, S \ P); children,
 *               parent links (the 7 leaves' too), union box (ascending leaf order), primitive count
 *               and "holds an object leaf" of the 6 slots are rewritten.
 * area_before and area_after are the objective over all trees before the first pass and after the
 * last, each reduced in a fixed order; with passes = 0 both are the objective of the clustered tree.
 * ------------------------------------------------------------------------------- */
typedef struct {
    int32_t passes;   /* 0 (default): off.  1 .. 8 */
    int32_t gamma;    /* 0: the built-in value, 7.  7 .. 2^20: least primitives under a restructured node */
    int32_t reserved[2];  /* 0 */
} lumo_wide_treelet_cfg;
/* cfg NULL: the defaults.  LUMO_ERR_INVALID for a NULL context, a field outside its range or a
 * non-zero reserved; the setting is then as it was. */
lumo_status lumo_scene_set_wide_treelet(void* ctx, const lumo_wide_treelet_cfg* cfg);

typedef struct {
    int32_t passes_used, reserved;
    int64_t tried, replaced;          /* treelets of 7 leaves over all passes; those that were replaced */
    double area_before, area_after;
    double treelet_ms;   /* HIP events around the passes; lumo_wide_build_info.build_ms holds them too,
                            lumo_wide_cluster_info.cluster_ms does not */
} lumo_wide_treelet_info;
/* Of the last upload.  LUMO_ERR_NO_SCENE before one. */
lumo_status lumo_scene_wide_treelet_info(void* ctx, lumo_wide_treelet_info* info);

/* ---------------------------------------------------------------------------------
 * Dynamic geometry: vertices updated in place, the wide BVH refit on the device (DESIGN.md §4g
 * "Refit").  Additions within ABI 10, found by dlsym.
 *
 * lumo_scene_update_vertices overwrites vertices first .. first + count - 1 of the uploaded scene
 * with xyz (3 * count doubles) and brings everything the wide mode (accel = 1) reads up to date: the
 * per-triangle soup, the leaf records, the child boxes of every node of every tree (world objects,
 * world lights, each BLAS), the world boxes of the instance leaves (from the exact f64 bounds of
 * their BLAS, through the builders' transform rule), max_abs and the staged LDS copies.  The
 * topology (refs, child counts, record order, roots, stack need, depth) stays.  A child box is
 * again the f32 box rounded outward from the exact f64 bounds of what lies beneath it, so a refit
 * tree walks like any valid tree; it is only as good a partition as the moved geometry lets the old
 * topology be (compare sah_cost with sah_build and rebuild with lumo_scene_upload when it has grown).
 * Works on a tree of either builder, with any cluster / treelet setting.  Synchronous.
 *
 * Refused, with nothing modified:
 *   LUMO_ERR_INVALID      NULL ctx or xyz, first < 0, count < 0, first + count > the scene's vertices,
 *                         a non-finite coordinate
 *   LUMO_ERR_NO_SCENE     before an upload
 *   LUMO_ERR_UNSUPPORTED  the scene's lumo_scene_info.accel is 0 (kd-trees and object BVHs cannot be
 *                         refit); a protected vertex given a value not bit-equal to its present one
 * A vertex is protected when a triangle of a light, or of an object that is no kd mesh (a Rectangle,
 * a single Triangle), uses it: the sampled light's own hit walks that light's kd-tree, and areas,
 * Rectangle parameters and the alias table are made on the host.  Values bit-equal to the present
 * ones are always accepted, so the whole vertex array of the moved scene may be passed.
 * Normals and uvs are not touched.
 * ------------------------------------------------------------------------------- */
lumo_status lumo_scene_update_vertices(void* ctx, int32_t first, int32_t count, const double* xyz);

typedef struct {
    int64_t changed;   /* vertices of the last accepted update whose value changed                      */
    int64_t updates;   /* accepted updates since the upload (0: the other fields but sah_build are 0)  */
    double refit_ms;   /* HIP events around the device work of the last update                         */
    double sah_cost;   /* after the last update, by lumo_wide_build_info.sah_cost's rule                */
    double sah_build;  /* of the tree as it was built, by the device's reduction: lumo_wide_build_info.
                          sah_cost itself for the device builder, within rounding of it for the host's;
                          0 before the first update                                                     */
    float max_abs;     /* the largest |box coordinate| after the last update                           */
    int32_t reserved;
} lumo_refit_info;
/* Of the last accepted update since the upload.  LUMO_ERR_NO_SCENE before an upload. */
lumo_status lumo_scene_refit_info(void* ctx, lumo_refit_info* info);

/* ---------------------------------------------------------------------------------
 * Motion: where each film sample's surface point was before the frame's vertex updates, for the
 * temporal denoiser (DESIGN.md §4g "Motion").  Additions within ABI 10, found by dlsym.
 *
 * lumo_scene_motion_mark copies the present vertex array into the context's "previous" vertices
 * (allocated by the first mark after an upload, dropped by the next upload and by lumo_destroy).
 * Per frame: mark, any number of lumo_scene_update_vertices calls, the renders.  Before the first
 * mark the previous vertices are the present ones, so all motion is exactly 0; with accel = 0
 * nothing can move and it stays 0.  Errors: LUMO_ERR_INVALID (NULL context), LUMO_ERR_NO_SCENE,
 * LUMO_ERR_OOM.
 *
 * Per sample (f64, never contracted, in this order): delta = 0 for a miss, a light, a sphere, a
 * Rectangle and a single Triangle (lumo_scene_update_vertices protects them).  For a hit on a kd
 * mesh, triangle tri with vertices A B C (present) and A' B' C' (previous), on the object's local
 * ray:
 *   bary         e / det of the accepted triangle test (triangle.rs:131-134)
 *   xi           (bary.x A + bary.y B) + bary.z C per component: the record's local p bit for bit
 *   xi'          the same expression of A' B' C'
 *   delta_local  xi' - xi
 *   delta        an instance: row r of its local-to-world m as a direction,
 *                ((m_r0 dx + m_r1 dy) + m_r2 dz) + m_r3 0; else delta_local
 * so the point's previous world position is p + delta.
 *   motion_w     sum w delta, sum w: the beauty film's filter weights summed in its order, channel
 *                3 the beauty tile's sum w bit for bit.  Consumers divide channels 0-2 by depth_w
 *                channel 1 (sum w hit): the motion averaged over the samples the depth is.
 * ------------------------------------------------------------------------------- */
lumo_status lumo_scene_motion_mark(void* ctx);
typedef struct {
    double* motion_w; /* 4 doubles per tile pixel, as rgb_w; NULL: skipped */
} lumo_motion_planes;
/* Per-sample records of one task, laid out as lumo_feature_dump's; a NULL array is skipped. */
typedef struct {
    double* bary;  /* 3 (zeros where delta is 0 by kind) */
    double* delta; /* 3 */
} lumo_motion_dump;
/* lumo_render_features with the motion plane from the same primary rays: `out` (n entries) may be
 * NULL, the feature planes are then not made; `motion` has n entries.  Errors as
 * lumo_render_features, with LUMO_ERR_INVALID for a NULL motion. */
lumo_status lumo_render_features_motion(void* ctx, const lumo_tile_task* tasks, size_t n, const lumo_feature_cfg* cfg,
                                        lumo_feature_planes* out, const lumo_motion_planes* motion);
/* Test hook: the per-sample motion records of one task, with the sampler of lumo_debug_set_sampler;
 * sample for sample those of lumo_debug_features. */
lumo_status lumo_debug_motion(void* ctx, const lumo_tile_task* task, lumo_motion_dump* dump);
/* lumo_denoise_temporal with the frame's motion plane (height x width x 4, assembled like the other
 * planes).  motion_w NULL: lumo_denoise_temporal itself, the same launches and bits.  Else
 *   step 1 gains  m = motion_w[0..2] / depth_w[1] per component, 0 where depth_w[1] = 0
 *   step 2 gains  P' = P + m per component
 *   step 3 uses   P' wherever it used P: c' = xf(world_to_camera', P'), z' from |P' - o'|
 * and everything after is unchanged.  Errors as lumo_denoise_temporal. */
lumo_status lumo_denoise_temporal_motion(void* ctx, const lumo_denoise_in* in, const double* motion_w,
                                         const lumo_camera_desc* camera, const lumo_denoise_cfg* cfg,
                                         const lumo_temporal_cfg* tcfg, double* rgb_out, double* variance_out,
                                         lumo_temporal_info* info);

/* Test hook: the wide BVH of the uploaded scene as it lies on the device, whichever builder made it.
 * Two calls: with only info (8 values: accel on, nodes, leaf records, stack, depth, objects root,
 * lights root, 0) for the sizes, then with the arrays (nodes x 128 B, records x 10 doubles, one
 * BLAS root per object and per light).  LUMO_ERR_NO_SCENE before an upload. */
lumo_status lumo_debug_wide_export(void* ctx, int64_t* info, void* nodes, double* tv, int32_t* obj_blas,
                                   int32_t* light_blas);

#ifdef __cplusplus
}
#endif
#endif /* LUMO_AMD_H */
