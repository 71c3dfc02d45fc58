/*
 * rt_abi.h — C ABI of the MI355X path-tracing hot path (go_raytracer_amd).
 *
 * Drop-in boundary for the reference's per-pixel render loop
 *     (*Camera).Render(world, lights hittable.Hittable)   internal/camera/camera.go:156
 * The reference has no FFI; the seam is its Go interfaces (Hittable
 * hittable.go:60-65, Material materials.go:19-27, Texture texture.go:10-12).
 * A cgo shim walks the Go object tree with the rt_new_* /
 * rt_mat_* / rt_tex_* constructors below — one call per Go constructor — and
 * then calls rt_scene_create + rt_render instead of Camera.Render.
 *
 * Conventions: every function returns RT_OK (0) or a negative RT_ERR_* code,
 * or a non-negative handle.  Nothing aborts the process (the reference calls
 * log.Fatal, camera.go:188, hittable.go:70, imageLoader.go:32-36); the message
 * of the last failure on the calling thread is in rt_last_error().
 * All inputs are copied; callers may free them after the call returns.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4

enum {
  RT_OK = 0,
  RT_ERR_INVALID = -1,     /* bad argument / handle */
  RT_ERR_UNSUPPORTED = -2, /* e.g. a BVH or transform used as a light (hittable.go:69-72) */
  RT_ERR_DEVICE = -3,      /* HIP runtime failure or no GPU */
  RT_ERR_OOM = -4,         /* out of memory; a device allocation that hipMalloc refuses with
                              hipErrorOutOfMemory, in every entry (the render, the BVH build and
                              rt_render_multi reported RT_ERR_DEVICE for it before) */
  RT_ERR_IO = -5
};

const char* rt_last_error(void);
int rt_abi_version(void);

/* Tuning overrides (A/B experiments and tests; the knobs and their measured defaults are
 * listed in DESIGN.md §6).  The library never reads the process environment: a knob
 * differs from its default only after the caller sets it here, and rt_scene_info.tuned /
 * rt_stats.tuned report how many knobs were set when the scene was created / the render
 * ran (the reference is configured through Camera fields only, camera.go:181-207).
 * value: a number as text (or a file path for RT_WAVE_TIMES, host|device|auto for
 * RT_BVH_BUILDER); NULL clears the knob; name NULL clears every knob.  Unknown names, text
 * that is not one whole number, and numbers outside the knob's range (e.g. RT_STEP_BUDGET
 * below 1) return RT_ERR_INVALID and leave the knob as it was.  Process-wide. */
int rt_tune_set(const char* name, const char* value);
/* The value knob `name` is set to: returns 0 when it is not set, else the value's length + 1
 * (the buffer size it needs), copying at most cap - 1 bytes and a NUL into buf when buf is not
 * NULL and cap > 0.  Unknown names return RT_ERR_INVALID. */
int rt_tune_get(const char* name, char* buf, int32_t cap);
/* Knob i's name and whether it may change image bits (the others move work only); returns
 * the number of knobs (i < 0: just the count). */
int rt_tune_list(int32_t i, const char** name, int32_t* changes_bits);
/* The record loop's layout matcher, as render uses it (host only, no device): counts = the pair
 * counts of a tiny scene's record groups {general, y-parallel, x, y, z axis-aligned, mixed-pair
 * code, box pairs}.  Returns the id (>= 1) of the compiled-in layout whose counts equal them
 * exactly, 0 when only the generic kernel takes them. */
int rt_brute_shape(const int32_t counts[7]);

/* ------------------------------------------------------------------------ */
/* Scene tree: one constructor per reference constructor.                    */
/* ------------------------------------------------------------------------ */
typedef struct rt_tree rt_tree;

int rt_tree_create(rt_tree** out);
int rt_tree_destroy(rt_tree* t);

/* Scene-construction randomness (the reference uses the global math/rand for
 * random scene content, main.go:38-75,107,155, and perlin tables,
 * perlin.go:20-31).  A per-tree splitmix64 stream replaces it. */
int rt_tree_seed(rt_tree* t, uint64_t seed);
double rt_tree_rand(rt_tree* t);             /* rand.Float64()        */
double rt_tree_rand_range(rt_tree* t, double lo, double hi); /* util.RangeRange utilities.go:12 */
int rt_tree_randn(rt_tree* t, int n);        /* rand.Intn(n)          */

/* textures — texture.go */
enum { RT_TEX_SOLID = 0, RT_TEX_CHECKER = 1, RT_TEX_IMAGE = 2, RT_TEX_NOISE = 3 };
enum { RT_NOISE_PERLIN = 1, RT_NOISE_MARBLE = 2, RT_NOISE_TURBULENT = 3 }; /* texture.go:88-95 */
int rt_tex_solid(rt_tree* t, double r, double g, double b);                 /* NewSolidColor texture.go:18 */
int rt_tex_checker(rt_tree* t, double scale, int even_tex, int odd_tex);    /* NewCheckerboard texture.go:37 */
/* NewImageTexture texture.go:66 with the image already decoded to RGB8
 * rows (RTImage.bdata layout imageLoader.go:52-62); w*h*3 bytes copied. */
int rt_tex_image(rt_tree* t, const uint8_t* rgb, int w, int h);
/* NewNoiseTextureWithType texture.go:108: perlin tables drawn from the tree RNG
 * in NewPerlin's order (perlin.go:20-31, 81-90). */
int rt_tex_noise(rt_tree* t, double scale, int variant);
/* same, with explicit tables (ranvec[256][3] doubles, perm[3][256]) */
int rt_tex_noise_tables(rt_tree* t, double scale, int variant, const double* ranvec,
                        const int32_t* perm);

/* materials — materials.go */
enum {
  RT_MAT_LAMBERTIAN = 0,
  RT_MAT_METAL = 1,
  RT_MAT_DIELECTRIC = 2,
  RT_MAT_DIFFUSE_LIGHT = 3,
  RT_MAT_ISOTROPIC = 4
};
int rt_mat_lambertian(rt_tree* t, int tex);                               /* NewTexturedLambertian :40 */
int rt_mat_metal(rt_tree* t, double r, double g, double b, double fuzz); /* NewMetal :65 */
int rt_mat_dielectric(rt_tree* t, double ior);                            /* NewDielectric :89 */
int rt_mat_diffuse_light(rt_tree* t, int tex);                            /* NewDiffuseLightTextured :139 */
int rt_mat_isotropic(rt_tree* t, int tex);                                /* NewIsotropicTexture :165 */

/* hittables — hittable.go, bvh.go, objects.go, transformation.go, medium.go */
enum {
  RT_NODE_LIST = 0,
  RT_NODE_BVH = 1,
  RT_NODE_SPHERE = 2,
  RT_NODE_QUAD = 3,
  RT_NODE_TRIANGLE = 4,
  RT_NODE_TRANSLATE = 5,
  RT_NODE_ROTATE_Y = 6,
  RT_NODE_MEDIUM = 7
};
int rt_new_list(rt_tree* t);                        /* NewHittableList hittable.go:84 */
int rt_list_add(rt_tree* t, int list, int obj);     /* HittableList.Add hittable.go:113 */
int rt_build_bvh(rt_tree* t, int list);             /* BuildBVH bvh.go:21 */
int rt_new_sphere(rt_tree* t, const double center[3], double radius, int mat); /* objects.go:23 */
int rt_new_motion_sphere(rt_tree* t, const double c1[3], const double c2[3], double radius,
                         int mat);                  /* NewMotionSphere objects.go:30 */
int rt_new_quad(rt_tree* t, const double Q[3], const double u[3], const double v[3],
                int mat);                           /* NewQuad objects.go:129 */
int rt_new_box(rt_tree* t, const double a[3], const double b[3], int mat); /* NewBox objects.go:208 */
/* NewTriangle / NewTriangleWithNormals / NewTexturedTriangle[WithNormals]
 * objects.go:257-316.  normals (9) and uv (6) may be NULL. */
int rt_new_triangle(rt_tree* t, const double v[9], const double* normals, const double* uv,
                    int mat);
/* bulk form for meshes: n triangles, returns a LIST node holding them */
int rt_new_triangles(rt_tree* t, int n, const double* v, const double* normals,
                     const double* uv, const int32_t* mats);
int rt_translate(rt_tree* t, int obj, const double offset[3]);  /* Translate transformation.go:20 */
int rt_rotate_y(rt_tree* t, int obj, double degrees);           /* RotateY transformation.go:48 */
int rt_constant_medium(rt_tree* t, int boundary, double density, int tex); /* medium.go:20 */

/* ------------------------------------------------------------------------ */
/* OBJ/MTL loader — LoadObjWithOptions internal/objLoader/objLoader.go:72-538, */
/* LoadMTL + ConvertToRaytracerMaterial mtlLoader.go:53-326.  Builds the same  */
/* triangles (bit-identical fp64 vertices/normals/uvs), the same materials and */
/* the same two Hittables as the Go loader: *model = BuildBVH(all triangles),  */
/* *lights = list of the emissive (and, with find_windows, dielectric) ones.   */
/* ------------------------------------------------------------------------ */
typedef struct {
  const char* name;   /* map_Kd / map_Ka string exactly as written in the MTL */
  const uint8_t* rgb; /* w*h*3, decoded by the caller (image.Decode imageLoader.go:34) */
  int32_t w, h;
} rt_obj_image;

typedef struct {                /* LoadObjOptions objLoader.go:18-29 */
  double scale_factor;          /* ScaleFactor */
  int32_t flip_yz;              /* FlipYZ */
  int32_t debug;                /* Debug: print the loader's diagnostics to stdout */
  int32_t ignore_normals;       /* IgnoreNormals */
  int32_t center;               /* Center (Position is applied only when set, :243-248) */
  int32_t flip_faces;           /* FlipFaces */
  int32_t default_material;     /* DefaultMaterial; -1 = nil -> Lambertian(.8,.8,.8) :88-90 */
  double position[3];           /* Position */
  int32_t ignore_mtl;           /* IgnoreMtl */
  int32_t find_windows;         /* FindWindows */
  /* image textures named by map_Kd / map_Ka: looked up here by exact name
   * first; otherwise the file is opened as written (binary PPM only). */
  int32_t n_images;
  int32_t _pad;
  const rt_obj_image* images;
} rt_obj_options;

typedef struct {
  int64_t n_vertices, n_normals, n_texcoords, n_triangles, n_lights;
  int32_t n_materials;      /* materials in the MTL library */
  int32_t default_material; /* material id used for faces without a known usemtl */
  double bounds_min[3], bounds_max[3], center[3]; /* after scale/flip, before centring */
} rt_obj_info;

int rt_obj_default_options(rt_obj_options* o); /* DefaultLoadOptions objLoader.go:32-45 */
int rt_load_obj(rt_tree* t, const char* filename, const rt_obj_options* opts, int* model,
                int* lights, rt_obj_info* info);
/* Same from memory (e.g. a Go embed.FS); mtl_text, when non-NULL, replaces the file
 * named by mtllib; filename (may be NULL) only resolves the mtllib directory. */
int rt_load_obj_memory(rt_tree* t, const char* obj_text, size_t obj_len, const char* mtl_text,
                       size_t mtl_len, const char* filename, const rt_obj_options* opts,
                       int* model, int* lights, rt_obj_info* info);

/* ------------------------------------------------------------------------ */
/* Read-only view of a tree (consumed by the CPU oracle and the cgo shim).  */
/* ------------------------------------------------------------------------ */
typedef struct {
  int32_t kind;  /* RT_NODE_* */
  int32_t mat;   /* material id (prims), phase material (medium) */
  int32_t a, b;  /* LIST/BVH: children[a .. a+b); TRANSLATE/ROTATE_Y: a = child;
                    MEDIUM: a = boundary; TRIANGLE: a = index into tris */
  double p[10];  /* SPHERE: c1[3] c2[3] r moving; QUAD: Q u v; TRANSLATE: off;
                    ROTATE_Y: degrees; MEDIUM: density */
} rt_node;

typedef struct {
  double v[9];   /* 3 vertices */
  double n[9];   /* vertex normals (if flags & 1) */
  double uv[6];  /* texture coords (if flags & 2) */
  int32_t flags; /* 1 = has vertex normals, 2 = has uv */
  int32_t mat;
} rt_tri;

typedef struct {
  int32_t kind;   /* RT_MAT_* */
  int32_t tex;    /* lambertian / light / isotropic */
  double albedo[3];
  double fuzz;
  double ior;
} rt_material;

typedef struct {
  int32_t kind;    /* RT_TEX_* */
  int32_t a, b;    /* CHECKER: even, odd; IMAGE: image id; NOISE: perlin id */
  int32_t variant; /* NOISE */
  double color[3]; /* SOLID */
  double scale;    /* CHECKER: inv_scale (= 1/scale as texture.go:39); NOISE: scale */
} rt_texture;

typedef struct {
  int32_t w, h;
  const uint8_t* rgb; /* w*h*3 */
} rt_image;

typedef struct {
  double ranvec[256][3];
  int32_t perm[3][256];
} rt_perlin;

typedef struct {
  const rt_node* nodes;
  int32_t n_nodes;
  const int32_t* children;
  int32_t n_children;
  const rt_tri* tris;
  int32_t n_tris;
  const rt_material* materials;
  int32_t n_materials;
  const rt_texture* textures;
  int32_t n_textures;
  const rt_image* images;
  int32_t n_images;
  const rt_perlin* perlins;
  int32_t n_perlins;
} rt_tree_view;

int rt_tree_get_view(const rt_tree* t, rt_tree_view* out);

/* ------------------------------------------------------------------------ */
/* Camera — public fields of Camera camera.go:26-36 + PositionCamera :65.    */
/* Zero means "use the reference default" exactly as initialize() :181-207. */
/* ------------------------------------------------------------------------ */
typedef struct {
  double aspect_ratio;        /* 0 -> 1.0 */
  int32_t width;              /* 0 -> 100 */
  int32_t samples_per_pixel;  /* 0 -> 100 (truncated to floor(sqrt)^2, camera.go:211) */
  int32_t max_depth;          /* 0 -> 10 */
  int32_t max_threads;        /* -N; unused by the GPU path (kept for API parity) */
  double vertical_fov;        /* 0 -> 90 */
  double defocus_angle;       /* 0 -> 0 */
  double focus_distance;      /* 0 -> 10 */
  double background[3];       /* Background (nil in Go == black here) */
  double max_contribution;    /* 0 -> 1.5 */
  double look_from[3];        /* PositionCamera; a never-positioned camera uses */
  double look_at[3];          /*   lookFrom (0,0,0), lookAt (0,0,-1), vup (0,1,0) */
  double vup[3];
  int32_t positioned;         /* 0 -> the defaults above */
  int32_t _pad;
} rt_camera;

/* Derived geometry, initialize() camera.go:179-253 (fp64). */
typedef struct {
  int32_t width, height, spp_sqrt, max_depth;
  double pixel_samples_scale, recip_spp_sqrt;
  double center[3], pixel00[3], delta_u[3], delta_v[3], defocus_u[3], defocus_v[3];
  double defocus_angle, max_contribution;
  double background[3];
} rt_camera_derived;

int rt_camera_derive(const rt_camera* cam, rt_camera_derived* out);

/* ------------------------------------------------------------------------ */
/* Flattened scene + render.                                                 */
/* ------------------------------------------------------------------------ */
typedef struct rt_scene rt_scene;

/* Flatten world/lights (transforms baked, media separated, light table built)
 * and build the device BVH (BuildBVH bvh.go:21-61 + the world list).  Scenes of
 * >= 65536 world prims build it on the calling thread's current HIP device (PLOC,
 * DESIGN.md "BVH"; the current device is left unchanged) when one is
 * present, otherwise with the host binned-SAH builder; the knobs RT_BVH_BUILDER
 * (host|device) and RT_BVH_DEVICE_MIN (rt_tune_set) override.  lights may be -1. */
int rt_scene_create(const rt_tree* t, int world, int lights, rt_scene** out);
int rt_scene_destroy(rt_scene* s);

typedef struct {
  int32_t n_spheres, n_quads, n_triangles;
  int32_t n_world_prims, n_media, n_lights;
  int32_t n_bvh_nodes, bvh_depth, max_leaf;
  int32_t n_materials, n_textures, n_images, n_perlins;
  int32_t medium_draws; /* total free-flight draws per vertex */
  int64_t device_bytes; /* scene bytes uploaded to HBM */
  int32_t features;     /* RT_FT_* bits the scene needs (selects the fused kernel) */
  int32_t bvh_builder;  /* 0: host binned SAH, 1: device PLOC (rt_scene_create) */
  int32_t tuned;        /* rt_tune_set knobs set when the scene was created (0: defaults) */
  int32_t _pad;
} rt_scene_info;

/* scene features (rt_scene_info.features, rt_stats.kernel_features) */
enum {
  RT_FT_SPHERE = 1, RT_FT_TRI = 2, RT_FT_METAL = 4, RT_FT_DIEL = 8, RT_FT_MEDIA = 16,
  RT_FT_CHECKER = 32, RT_FT_IMAGE = 64, RT_FT_NOISE = 128,
  RT_FT_BOX = 256 /* box leaves (NewBox as one BVH leaf; scenes above 256 world prims) */
};
int rt_scene_info_get(const rt_scene* s, rt_scene_info* out);

/* BVH export for structural tests: nodes as 16 floats
 * {b0min[3], b0max[3], b1min[3], b1max[3], child0 bits, child1 bits, 0, 0},
 * leaf child encoding documented in DESIGN.md.  Pass NULL to query counts. */
int rt_scene_export_bvh(const rt_scene* s, float* nodes, int32_t* n_nodes, uint32_t* prim_refs,
                        int32_t* n_refs, uint32_t* root);
/* the wide tree large scenes render with: BVH8 nodes as 32 floats
 * (rt_device.h "BVH8 node", 16-bit planes) and the prim ref of each of its leaf
 * records; 0 nodes when the scene has none.  Pass NULL to query counts. */
int rt_scene_export_bvh8(const rt_scene* s, float* nodes, int32_t* n_nodes, uint32_t* refs8,
                         int32_t* n_refs8);
/* world-prim float AABBs in prim-ref order (6 floats each) */
int rt_scene_export_prim_bounds(const rt_scene* s, float* bounds, int32_t* n);
/* the compressed BVH4 the fused kernels read through L1/L2 (rt_device.h "compressed BVH4
 * node", 64-B items: nodes with fp16 child planes and single-prim leaf records; 0 items when
 * the scene's tree is not encodable) and the BVH4 it encodes (8 float4 per node), for
 * structural tests.  NULL pointers query the counts. */
int rt_scene_export_qbvh(const rt_scene* s, float* items, int32_t* n_items, float* nodes4,
                         int32_t* n_nodes4, uint32_t* root4);
/* the record loop's pair array as uploaded for scenes small enough to have one (rt_device.h
 * "record-loop pair layout"): 4 float4 per slot, then shade_n float4 of the lean kernel's
 * shade table (0: none), so 16 * n_slots + 4 * shade_n floats; the seven layout counts in
 * rt_brute_shape's order; the boxes tested as slabs.  n_slots = 0 when the scene is too large
 * to have pairs.  NULL pointers query the sizes. */
int rt_scene_export_records(const rt_scene* s, float* pairs, int32_t* n_slots, int32_t counts[7],
                            int32_t* shade_n, int32_t* n_boxes);
/* structural test export: a tree over caller-supplied boxes (n x 6 floats: lo xyz, hi xyz),
 * built by the unchanged builder of rt_scene_create -- builder 0: the host binned SAH, 1: the
 * device PLOC on the calling thread's current device (RT_ERR_DEVICE without one) -- with prim i
 * = box i and no padding, so a test can put boxes on an exact lattice.  Outputs as
 * rt_scene_export_bvh (nodes, refs: leaf position -> box index, root), rt_scene_export_qbvh's
 * BVH4 (nodes4, root4) and rt_scene_info's bvh_depth and max_leaf.  n_nodes and n_nodes4 are
 * at most max(n - 1, 0) and n_refs is n; NULL pointers query the counts (the tree is built
 * either way).  n = 0 and n = 1 follow the builder: the host one gives an empty tree
 * (root PRIM_NONE) and a single leaf, the device one RT_ERR_INVALID below two boxes. */
int rt_bvh_build_boxes(const float* boxes, int32_t n, int32_t builder, float* nodes,
                       int32_t* n_nodes, uint32_t* refs, int32_t* n_refs, uint32_t* root,
                       float* nodes4, int32_t* n_nodes4, uint32_t* root4, int32_t* bvh_depth,
                       int32_t* max_leaf);
/* the lean light kind of the scene's light list as the host matcher decides it at upload (no
 * device): 0 = any list (the general light code), 1 = one quad light of weight 1 with unit
 * normal +-e_y in a lean-set scene (RT_FT features 0) of non-negative colours.  For a kind
 * >= 1, block receives the light as the record-loop kernel of that kind reads it, n_floats
 * (20) floats: [0..2] Q, [3] D / n_y, [4..6] A = v x w, [7] area, [8..10] B = w x u,
 * [12..14] u, [16..18] v ([11], [15], [19] are 0); all zero for kind 0.  NULL pointers query
 * the sizes. */
int rt_scene_lean_light(const rt_scene* s, int32_t* kind, float* block, int32_t* n_floats);
/* the lean light kind a fused render of the scene on `device` launches with now (uploads the
 * scene there on first use): the matcher's kind when the record-loop kernel compiled for it
 * takes the scene and RT_LEAN_LIGHT is not 0, else 0.  A render whose background has a
 * negative channel takes kind 0 whatever this returns. */
int rt_scene_plan_light(rt_scene* s, int device, int32_t* kind);
/* the emitter slot of the scene's record layout (host code only, no device): the position, in
 * the slot order of rt_scene_export_records' pair array (2 * pair + half), of the scene's one
 * emissive record, when the record-loop kernel may take "the hit scatters" from the winning
 * slot alone and so draw a vertex's random numbers before the winner is resolved -- a listed
 * layout (rt_brute_shape 1 or 2), lean light kind 1, exactly one emissive quad in the world,
 * which is the light list's quad and not a face of a box tested as slabs.  -1 otherwise. */
int rt_scene_lean_emitter(const rt_scene* s, int32_t* slot);
/* 1 when a fused render of the scene on `device` launches the early-draw record-loop kernel
 * now (uploads the scene there on first use): the lean light kind's kernel is taken
 * (rt_scene_plan_light), the scene has an emitter slot, its layout is rt_brute_shape 1 (the
 * one layout with such a kernel) and RT_LEAN_EARLY_DRAW is not 0; else 0.  A render whose background has a negative channel takes the general kernel whatever
 * this returns. */
int rt_scene_plan_early(rt_scene* s, int device, int32_t* early);
/* ... and 1 when that launch takes the early-draw kernel's lean-cost twin (the default where the
   early-draw kernel is taken; RT_LEAN_COST=0 keeps the early-draw kernel itself), else 0 */
int rt_scene_plan_cost(rt_scene* s, int device, int32_t* cost);

enum {
  RT_FLAG_PROFILE = 1,     /* time every kernel with HIP events */
  RT_FLAG_GATHER_RCCL = 2  /* rt_render_multi: gather the shares with one RCCL ncclGather
                              (communicators over the device list, cached per scene;
                              the devices must be distinct) instead of peer copies */
};

/* execution strategy of the same per-vertex code (DESIGN.md "Kernels"):
 *   WAVEFRONT: queue-driven extend / shade kernels, path state in HBM (SoA)
 *   FUSED:     one persistent kernel, path state in registers
 *   AUTO:      the faster one for the scene */
enum { RT_MODE_AUTO = 0, RT_MODE_WAVEFRONT = 1, RT_MODE_FUSED = 2 };

typedef struct {
  uint64_t seed;       /* render_seed */
  int32_t device;      /* HIP device ordinal */
  int32_t rank;        /* row-interleaved shard: rows r with r % nranks == rank */
  int32_t nranks;
  int32_t path_slots;  /* wavefront capacity; 0 = auto */
  int32_t chunk;       /* samples per work chunk; 0 = auto */
  int32_t flags;       /* RT_FLAG_* */
  int32_t mode;        /* RT_MODE_* */
  void* stream;        /* hipStream_t to enqueue on; NULL = library stream */
  /* path trace of one sample (debugging): when trace_out != NULL the vertices
   * of sample trace_sample of global pixel trace_pixel are written as 12 floats
   * {o.xyz, time, d.xyz, vertex, t, u, v, prim-ref bits} per world.Hit call,
   * up to trace_cap vertices; unused entries have vertex = -1. */
  int64_t trace_pixel;
  int32_t trace_sample;
  int32_t trace_cap;
  float* trace_out;
  /* rt_progress granularity: the fused render runs as this many launches over
   * consecutive chunk ranges (same image, bit for bit) and rt_progress advances
   * as each completes.  0/1 = one launch, progress only reports start and end. */
  int32_t progress_slices;
  int32_t _pad3;
} rt_render_opts;

typedef struct {
  uint64_t samples;      /* W*rows*spp_sqrt^2 rendered by this call */
  uint64_t segments;     /* closest-hit queries (world.Hit calls, camera.go:300) */
  uint64_t stack_pushes; /* clamp-vertex weights stored (0 unless built with RT_COUNT_PUSHES) */
  uint64_t extend_rays;  /* total rays processed by extend launches */
  uint64_t shade_rays;
  double ms_total;       /* render wall time (host, incl. sync) */
  double ms_extend;      /* summed extend-kernel time (RT_FLAG_PROFILE) */
  double ms_shade;
  double ms_other;
  int32_t n_extend_launches;
  int32_t n_shade_launches;
  int32_t iterations;
  int32_t rows;          /* rows rendered by this rank */
  int32_t mode;          /* RT_MODE_* actually used */
  int32_t path_slots;    /* concurrent paths (wavefront slots / fused lanes) */
  double ms_fused;       /* fused-kernel time (RT_FLAG_PROFILE) */
  int32_t kernel_features; /* RT_FT_* set compiled into the fused kernel that ran */
  int32_t scene_features;  /* RT_FT_* set the scene needs */
  int32_t tree_width;      /* tree the kernels traversed: 0 none (record loop), 2 BVH2, 4 BVH4,
                              5 BVH4 with 64-B compressed nodes (large trees) */
  int32_t lds_scene;       /* 1: nodes (and leaf records) ran from the LDS cache */
  int32_t chunk_samples;   /* samples per work chunk (opts.chunk or the adaptive choice) */
  int32_t record_boxes;    /* boxes the record loop tested as one slab test each (0: none) */
  /* sample channels with |v| >= 2^31 / spp_sqrt^2 (outside the exact fixed-point pixel
   * sum; added in fp64 instead — the image is then order-dependent in those pixels) */
  uint64_t overflow_samples;
  int32_t tuned;           /* rt_tune_set knobs set when the render ran (0: defaults) */
  int32_t chunk_records;   /* 1: per-chunk sum records, 0: pixel atomics (record buffer
                              over its cap or not allocatable: same image) */
} rt_stats;

/* Render this rank's rows; out_rgb (host) receives linear mean RGB
 * [rows][W][3] fp32, rows = rows r with r % nranks == rank in increasing order.
 * Replaces (*Camera).Render's pixel loop, camera.go:156 -> :90-153 (one process,
 * one device; rank/nranks = the row partition of camera.go:119-122 across processes).
 * Threading: an rt_scene keeps one device copy per device ordinal and one set of
 * render buffers per device; rt_render / rt_render_device may run concurrently from
 * different threads for DIFFERENT devices of one scene; calls for the same device
 * serialise (the second waits for the first). */
int rt_render(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts, float* out_rgb,
              rt_stats* stats);
/* Same, but out_rgb is a device pointer on opts->device (e.g. a torch tensor);
 * work is enqueued on opts->stream and the call returns after it completes. */
int rt_render_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                     float* out_rgb_device, rt_stats* stats);

/* Render the WHOLE image on n devices from one process (the north_star's 8-GPU tile
 * split, camera.go:119-122 row partition): device devices[i] renders rows
 * r % n == i, each share on its own host thread, stream and render buffers (a
 * device may repeat: {0, 0, 0} renders three shares on device 0); the shares are
 * copied to devices[0] (peer copies over xGMI) and de-interleaved there by a kernel.
 * out_rgb (host) receives [H][W][3]; the _device form writes a device pointer on
 * devices[0].  The image is bit-identical to rt_render's for any n (per-sample
 * fixed-point pixel sums).  opts->rank/nranks must be 0/1 and opts->stream NULL;
 * stats sum samples/segments over shares, ms_fused is the slowest share's.
 * opts->flags & RT_FLAG_GATHER_RCCL: each share renders into a padded send buffer on
 * its device and ONE ncclGather (RCCL over xGMI, root devices[0]) collects them, the
 * survey's collective for this step; same image bits.
 * One rt_render_multi per scene at a time (a second call waits). */
int rt_render_multi(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                    const int32_t* devices, int32_t n, float* out_rgb, rt_stats* stats);
int rt_render_multi_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                           const int32_t* devices, int32_t n, float* out_rgb_device,
                           rt_stats* stats);

/* Progress of the render in flight on scene s (the reference's progress bar,
 * camera.go:106-108 + internal/progress): may be polled from any thread while
 * rt_render blocks in another.  *total = samples of the current (or last)
 * render; *done = samples of the completed slices (opts.progress_slices), or
 * for rt_render_multi the samples of the completed shares, and *total once the
 * render returned.  A render refused before it starts leaves no render in
 * flight. */
int rt_progress(const rt_scene* s, uint64_t* done, uint64_t* total);

/* Output: PrintColor vec/color.go:23-46 (NaN->0, sqrt gamma, clamp .99999, x256). */
int rt_quantize(const float* rgb, int64_t n_pixels, uint8_t* out);
/* PPM P3 text exactly as camera.go:160 + PrintColor; returns bytes written
 * (call with out = NULL to size). */
int64_t rt_format_ppm(const float* rgb, int w, int h, char* out, int64_t cap);

/* On-device output (HIP): the same PrintColor bytes / P3 text, produced by kernels
 * from an image already in HBM (rgb_dev: device fp32 [n][3] on `device`; out_dev:
 * device memory; stream: hipStream_t or NULL).  The calls return after the work
 * completes.  rt_format_ppm_device returns the byte count (out_dev = NULL to size). */
int rt_quantize_device(const float* rgb_dev, int64_t n_pixels, uint8_t* out_dev, int device,
                       void* stream);
int64_t rt_format_ppm_device(const float* rgb_dev, int w, int h, char* out_dev, int64_t cap,
                             int device, void* stream);

/* ------------------------------------------------------------------------ */
/* Feature buffers (first hit of the render's own camera rays) and the       */
/* edge-avoiding a-trous denoiser they guide (DESIGN.md "Feature buffers and */
/* denoiser").  Added without an ABI version change: detect by the symbols.  */
/* ------------------------------------------------------------------------ */
typedef struct {          /* any pointer may be NULL = not wanted */
  float*   albedo;        /* [rows][W][3] */
  float*   normal;        /* [rows][W][3] world space, facing the ray; 0 on a miss */
  float*   depth;         /* [rows][W]    t * |d| from the ray origin; 0 on a miss */
  int32_t* material;      /* [rows][W]    RT_MAT_* of sample 0's hit, -1 on a miss */
} rt_aov;

/* The feature ray of sample j of a pixel is exactly the camera ray rt_render gives that
 * sample (same seed, RT_STREAM_CAMERA draw, stratum, defocus and time); the buffers hold
 * the mean over samples 0 .. n_samples-1 (0 means 1; more than spp_sqrt^2 is
 * RT_ERR_INVALID), material is sample 0's.  Rows follow opts->rank / nranks as
 * rt_render's.  The hit is the closest WORLD surface, evaluated as the render's shading
 * evaluates it; constant media are transparent to the feature pass (a smoke volume shows
 * the surface behind it; rt_render_aov_media below traces them).  Albedo: Lambertian / isotropic = the texture at the hit, metal =
 * its albedo, dielectric = (1,1,1), diffuse light = its emission when front-facing else 0,
 * miss = the camera background.  Two calls give identical bits.  stats (may be NULL):
 * samples and segments count the feature rays, tree_width the structure traversed (the one
 * rt_render's fused kernel takes for the scene), ms_total the wall time.
 * rt_render_aov: out_host holds host pointers; rt_render_aov_device: pointers on
 * opts->device, work enqueued on opts->stream (NULL: a library stream), returns after it
 * completes. */
int rt_render_aov(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                  int32_t n_samples, const rt_aov* out_host, rt_stats* stats);
int rt_render_aov_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                         int32_t n_samples, const rt_aov* out_device, rt_stats* stats);

typedef struct {
  int32_t iterations;     /* 0 -> 5; 1..8 */
  int32_t demodulate;     /* 1: filter rgb / max(albedo, 1e-3), multiply back after */
  float sigma_color;      /* 0 -> 0.5  (halved every iteration) */
  float sigma_normal;     /* 0 -> 0.3 */
  float sigma_depth;      /* 0 -> 0.02 (relative to the pixel's depth) */
  int32_t _pad;
} rt_denoise_opts;

/* Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) of a linear
 * RGB image [h][w][3], guided by feat (albedo / normal / depth as rt_render_aov writes them
 * for the same view; material is not read).  A pure image operation: no scene.  Iteration
 * i = 0 .. iterations-1 takes the 5 x 5 taps (dx, dy) in {-2..2}^2 * 2^i with the B3 kernel
 * h (x) h, h = [1/16, 1/4, 3/8, 1/4, 1/16], each weighted by
 *   exp(-|c_p - c_q|^2 / (sigma_color 2^-i)^2) exp(-|n_p - n_q|^2 / sigma_normal^2)
 *   exp(-(d_p - d_q)^2 / (sigma_depth max(d_p, 1e-6))^2)
 * (c from the previous iteration), skipping taps outside the image and pixels with a
 * non-finite colour, renormalised by the weights used; non-finite pixels pass through
 * unchanged.  feat->normal / feat->depth NULL switches that weight off; feat may be NULL
 * unless demodulate is set, which needs feat->albedo (else RT_ERR_INVALID).  out may alias
 * rgb.  opts NULL: the defaults.  rt_denoise: host pointers, staged through the device
 * (device 0); rt_denoise_device: device pointers on `device`, enqueued on `stream`
 * (hipStream_t or NULL), returns after the work completes. */
int rt_denoise(const float* rgb, const rt_aov* feat, int w, int h, const rt_denoise_opts* opts,
               float* out);
int rt_denoise_device(const float* rgb_dev, const rt_aov* feat_dev, int w, int h,
                      const rt_denoise_opts* opts, float* out_dev, int device, void* stream);

typedef struct {
  int32_t iterations;     /* 0 -> 5; 1..8 */
  int32_t demodulate;     /* 1: filter rgb / max(albedo, 1e-3), multiply back after */
  float sigma_lum;        /* 0 -> 1.0  (in standard deviations; the same in every iteration) */
  float sigma_normal;     /* 0 -> 0.3 */
  float sigma_depth;      /* 0 -> 0.02 (relative to the pixel's depth) */
  int32_t _pad;
} rt_denoise_var_opts;

/* The a-trous filter above with a variance-guided colour weight (the edge-stopping function of
 * Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017).  var [h][w] is the
 * variance of the mean luminance of rgb, as rt_accum_resolve writes it.  Added without an ABI
 * version change: detect by the symbols.  With Y(x) = 0.2126 x.r + 0.7152 x.g + 0.0722 x.b:
 *   prep: a pixel is valid when its three colour channels and its var are finite.  With
 *     a = max(albedo, 1e-3) per channel, c = rgb / a and v = var / Y(a)^2 when demodulating
 *     (exact for a grey albedo, an approximation otherwise: the variance of the luminance of
 *     rgb / a is not the variance of the luminance of rgb over Y(a)^2 when a's channels
 *     differ), else c = rgb, v = var; then v = max(v, 0).  Invalid pixels: c = 0, v = 0.
 *   iteration i = 0 .. iterations-1, step s = 2^i:
 *     g(p) = sum k3(dx) k3(dy) v(q) / sum k3(dx) k3(dy) over the 3 x 3 adjacent pixels
 *       q = p + (dx, dy), dx, dy in {-1, 0, 1} whatever s, k3 = [1/4, 1/2, 1/4], both sums over
 *       the taps inside the image and valid; none: g = 0.
 *     the 25 taps q = p + (dx, dy) s, dx, dy in {-2..2}, get the weight
 *       w = h(dx) h(dy) exp(-( |Y(c_p) - Y(c_q)| / (sigma_lum sqrt(g(p)) + 1e-6)
 *                             + |n_p - n_q|^2 / sigma_normal^2
 *                             + (d_p - d_q)^2 / (sigma_depth max(d_p, 1e-6))^2 ))
 *       for valid q inside the image, else 0 (h the B3 kernel above; a NULL normal / depth
 *       buffer switches its term off).
 *     c'(p) = sum w c_q / sum w,  v'(p) = sum w^2 v_q / (sum w)^2;  an invalid p keeps c and v.
 *   output: out = c a and var_out = v Y(a)^2 when demodulating, else c and v; invalid pixels
 *     pass rgb and var through bit for bit.
 * out may alias rgb; var_out may be NULL and may alias var.  Argument checks as rt_denoise's
 * (before any device is touched), and a NULL var is RT_ERR_INVALID. */
int rt_denoise_var(const float* rgb, const float* var, const rt_aov* feat, int w, int h,
                   const rt_denoise_var_opts* opts, float* out, float* var_out);
int rt_denoise_var_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev,
                          int w, int h, const rt_denoise_var_opts* opts, float* out_dev,
                          float* var_out_dev, int device, void* stream);

/* ------------------------------------------------------------------------ */
/* Emission split (DESIGN.md "Emission split"): what a directly seen light   */
/* contributes to a pixel, kept out of the filters.  Added without an ABI    */
/* version change: detect by the symbols.                                    */
/* ------------------------------------------------------------------------ */
typedef struct {            /* any pointer may be NULL = not wanted */
  float* emission;          /* [rows][W][3] */
  float* surface_albedo;    /* [rows][W][3] */
  float* coverage;          /* [rows][W]    */
} rt_aov_emit;

/* rt_render_aov with three more buffers.  The ray and the hit evaluation of sample j are
 * rt_render_aov's.  Let L_j be true when the closest world hit of sample j is an
 * RT_MAT_DIFFUSE_LIGHT seen from its front face.  Over samples 0 .. n-1:
 *   emission       = mean of E_j, E_j = the light's texture at the hit when L_j, else 0: exactly
 *                    what such a camera sample adds to the render.  It is NOT clamped: a
 *                    light does not scatter, so rayColor returns its emission (camera.go:312-314)
 *                    before the clampContribution of camera.go:330, which only a scattering
 *                    vertex reaches; MaxContribution does not enter
 *   surface_albedo = mean of A_j, A_j = rt_render_aov's albedo of the sample when !L_j (a miss
 *                    = the background, a back-facing light = 0), 0 when L_j
 *   coverage       = (float)count(L_j) / (float)n, a true division: exactly 1.0f when every
 *                    sample sees the light
 * out (may be NULL) takes rt_render_aov's four buffers, bit-identical to that call's.  Two
 * calls give identical bits.  A NULL emit, or out and emit together without any buffer, is
 * RT_ERR_INVALID (checked before any device is touched); otherwise the rules, the structures
 * traversed and the stats are rt_render_aov's. */
int rt_render_aov_emit(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                       int32_t n_samples, const rt_aov* out_host, const rt_aov_emit* emit_host,
                       rt_stats* stats);
int rt_render_aov_emit_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                              int32_t n_samples, const rt_aov* out_device,
                              const rt_aov_emit* emit_device, rt_stats* stats);

/* ------------------------------------------------------------------------ */
/* Media in the feature pass (DESIGN.md "Media in the feature pass"): the    */
/* first EVENT of a camera sample, which in a constant medium is a scatter,  */
/* not the surface behind it.  Opt-in and added without an ABI version       */
/* change: detect by the symbols.                                            */
/* ------------------------------------------------------------------------ */
typedef struct {
  float* scatter;           /* [rows][W]; may be NULL */
} rt_aov_media;

/* rt_render_aov_emit with the constant media traced.  The ray of sample j is rt_render_aov's and
 * its closest world hit is found as there (triangle refinement included).  Then the media are
 * laid over that hit exactly as the render's vertex 0 lays them: the free-flight draws are the
 * render's own, a pure function of (seed, pixel, sample j, vertex 0, the spare word of the
 * sample's camera draw), so the feature ray scatters exactly where the render's sample does.
 * The first event of sample j is whichever is closer; let M_j be true when it is a medium.
 *   M_j false: everything is as in rt_render_aov / rt_render_aov_emit for that sample.
 *   M_j true:  material kind = the kind of the medium's phase material (RT_MAT_ISOTROPIC);
 *              albedo = that material's texture at p = o + t d with u = v = 0, as the render's
 *              shading evaluates a medium hit; normal = (0, 0, 0), a volume has no shading
 *              normal; depth = t |d|; L_j = false, E_j = 0, A_j = the albedo.
 *   scatter  = (float)count(M_j) / (float)n, a true division as coverage's: exactly 0 where no
 *              sample scattered, exactly 1 where all did.
 * The buffers are means over samples 0 .. n-1 summed in fp32 in sample order, material is
 * sample 0's.  A miss behind a scatter is a medium event (depth > 0, the albedo is not the
 * background).  A pixel none of whose samples scattered has rt_render_aov's bits.  Two calls give
 * identical bits.  For a scene without media the call runs rt_render_aov_emit's kernels: every
 * plane has that call's bits and scatter is 0.
 * media must not be NULL (it selects the mode); out and emit may be NULL; RT_ERR_INVALID when no
 * buffer at all is wanted (every argument check comes before any device is touched).  Otherwise
 * the rules, the structures traversed and the stats are rt_render_aov's: segments count the
 * feature rays, not the media tests. */
int rt_render_aov_media(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                        int32_t n_samples, const rt_aov* out_host, const rt_aov_emit* emit_host,
                        const rt_aov_media* media_host, rt_stats* stats);
int rt_render_aov_media_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                               int32_t n_samples, const rt_aov* out_device,
                               const rt_aov_emit* emit_device, const rt_aov_media* media_device,
                               rt_stats* stats);

/* ------------------------------------------------------------------------ */
/* Specular chains in the feature pass (DESIGN.md "First diffuse-hit         */
/* guides"): the features of the first non-specular vertex behind mirrors    */
/* and glass.  Opt-in and added without an ABI version change: detect by the */
/* symbols.                                                                  */
/* ------------------------------------------------------------------------ */
typedef struct {
  int32_t max_bounces;      /* the last vertex a chain may reach; 0 -> 8; 0 .. 64 */
  float max_fuzz;           /* a metal is specular up to this fuzz; 0: perfect mirrors only */
} rt_aov_spec_opts;

typedef struct {
  float* bounces;           /* [rows][W]; may be NULL */
} rt_aov_spec;

/* rt_render_aov following perfectly specular vertices.  Sample j starts as rt_render_aov's: the
 * same camera ray, the same closest world hit, the same triangle refinement, constant media
 * transparent.  That hit is vertex 0 (the vertex the render's camera ray hits, whose scatter
 * draw is RT_STREAM(0, 0)).
 * Chain rule.  While vertex k is specular -- a dielectric, or a metal whose fuzz is <= max_fuzz
 * -- the sample scatters there exactly as the render's path does and the next segment is traced
 * with t_min = 0.001 from the hit point snapped onto its surface:
 *   dielectric: ri = 1 / ior on a front face, ior on a back face; total internal reflection, or
 *               Schlick's reflectance > word [0] of rt_rng_draw(seed, gpix, j, RT_STREAM(k, 0))
 *               as a unit float, reflects the unit direction; else it is refracted.
 *   metal:      unit(reflect(d, n)) + fuzz * the unit vector of words [2] and [3] of that call.
 * The chain's terminal vertex is the first of: a vertex that is not specular; a miss; a metal
 * whose scattered direction s has dot(s, n) <= 0 (it absorbs); vertex K = max(0, min(max_bounces,
 * MaxDepth - 1)), whatever it is.  With T the product of the attenuations of the specular
 * vertices passed (the metal's albedo; 1 for a dielectric), sample j contributes
 *   albedo   = T * the terminal's albedo by rt_render_aov's rules (lights and back faces
 *              included); T * the background on a miss
 *   normal   = the terminal's normal facing its own ray; 0 on a miss
 *   depth    = the sum of t |d| over the chain's segments up to the terminal; 0 when the terminal
 *              is a miss (no surface, as for the first hit)
 *   material = sample 0's terminal kind, -1 on a miss
 *   bounces  = the number of specular vertices passed
 * and the buffers are the means over samples 0 .. n-1 summed in fp32 in sample order (bounces: an
 * exact count divided once, exactly 0 where no sample left its first hit).  A sample that passed
 * no vertex contributes rt_render_aov's values, so a pixel with bounces == 0 has rt_render_aov's
 * bits in all four planes.  Two calls give identical bits.
 * spec must not be NULL (it selects the mode); spec_opts NULL = the defaults; out may be NULL.
 * RT_ERR_INVALID, before any device is touched: a NULL spec; no buffer wanted at all;
 * max_bounces < 0 or > 64; a negative or non-finite max_fuzz; then rt_render_aov's refusals.
 * The emission split and the media mode do not combine with this one.  The structures traversed
 * and the stats are rt_render_aov's, except that segments counts every segment traced: the
 * camera rays' and one per specular vertex passed. */
int rt_render_aov_spec(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                       int32_t n_samples, const rt_aov_spec_opts* spec_opts, const rt_aov* out_host,
                       const rt_aov_spec* spec_host, rt_stats* stats);
int rt_render_aov_spec_device(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                              int32_t n_samples, const rt_aov_spec_opts* spec_opts,
                              const rt_aov* out_device, const rt_aov_spec* spec_device,
                              rt_stats* stats);

/* rt_denoise / rt_denoise_var in split mode: the emission is subtracted before the filter and
 * added back after it, and the filter demodulates by the albedo of the surfaces the pixel
 * covers.  All three emit buffers are required (else RT_ERR_INVALID); feat->albedo is not read
 * and feat may be NULL.  The definition is the parent's with exactly these changes:
 *   valid pixel: the parent's rule, and emission finite, and coverage < 1.
 *   prep: a = max(surface_albedo, 1e-3) per channel, c = (rgb - emission) / a and
 *     v = max(var / Y(a)^2, 0) when demodulating; else c = rgb - emission, v = max(var, 0).
 *   iterations: unchanged (invalid taps are skipped as they are in the parent).
 *   output, valid pixels: out = c a + emission (c + emission when not demodulating),
 *     var_out = v Y(a)^2 (v when not demodulating): the emission is deterministic and adds no
 *     variance.
 *   output, invalid pixels (those with coverage 1 included): rgb and var pass through bit for
 *     bit, also when out aliases rgb and var_out aliases var.
 * With emission = 0, coverage = 0 and surface_albedo = albedo the result is the parent's. */
int rt_denoise_emit(const float* rgb, const rt_aov* feat, const rt_aov_emit* emit, int w, int h,
                    const rt_denoise_opts* opts, float* out);
int rt_denoise_emit_device(const float* rgb_dev, const rt_aov* feat_dev,
                           const rt_aov_emit* emit_dev, int w, int h,
                           const rt_denoise_opts* opts, float* out_dev, int device, void* stream);
int rt_denoise_var_emit(const float* rgb, const float* var, const rt_aov* feat,
                        const rt_aov_emit* emit, int w, int h, const rt_denoise_var_opts* opts,
                        float* out, float* var_out);
int rt_denoise_var_emit_device(const float* rgb_dev, const float* var_dev, const rt_aov* feat_dev,
                               const rt_aov_emit* emit_dev, int w, int h,
                               const rt_denoise_var_opts* opts, float* out_dev,
                               float* var_out_dev, int device, void* stream);

/* ------------------------------------------------------------------------ */
/* Progressive pass accumulator (DESIGN.md "Pass accumulator"): the exact    */
/* sum of any number of render passes of one camera, kept on the device,     */
/* with a per-pixel variance.  Added without an ABI version change: detect   */
/* by the symbols.                                                           */
/* ------------------------------------------------------------------------ */
typedef struct rt_accum rt_accum;

/* An accumulator for (scene, camera, opts' row share) on opts->device, with no pass yet.
 * The camera and device, rank / nranks, mode, chunk, path_slots, flags & RT_FLAG_PROFILE,
 * stream and progress_slices of opts (NULL: the defaults) are fixed here; opts->seed is
 * ignored (every pass brings its own) and opts->trace_out must be NULL.  max_passes: the most
 * passes it will take, 0 = 1024; negative, or spp_sqrt^2 * max_passes >= 2^31, is
 * RT_ERR_INVALID.  Arguments are checked before any device is touched.  About 76 bytes of
 * device memory per pixel of the share (plus 16 for rt_accum_resolve's staging), allocated
 * here; no call below allocates but rt_accum_set_features.  The scene owns its accumulators: rt_scene_destroy frees
 * those still alive (their handles are dead after it), rt_accum_destroy frees one early.
 * Calls on one accumulator serialise; passes and rt_render calls of one scene may interleave
 * (a pass holds the same per-device lock as rt_render while it runs). */
int rt_accum_create(rt_scene* s, const rt_camera* cam, const rt_render_opts* opts,
                    int32_t max_passes, rt_accum** out);
int rt_accum_destroy(rt_accum* a);
/* back to no passes; nothing is reallocated */
int rt_accum_reset(rt_accum* a);
/* One pass: exactly the samples rt_render computes for the accumulator's camera and options
 * with opts->seed = seed, added to the per-pixel sums as 2^-32 fixed-point integers, so the
 * sums do not depend on the order of the passes.  Samples with |v| >= 2^31 / (spp_sqrt^2 *
 * max_passes) are summed in fp64 beside them and counted in stats->overflow_samples, as
 * rt_render does above 2^31 / spp_sqrt^2.  stats (may be NULL) is the pass's own rt_stats.
 * A pass beyond max_passes returns RT_ERR_INVALID and changes nothing. */
int rt_accum_add(rt_accum* a, uint64_t seed, rt_stats* stats);
/* rgb [rows][W][3]: the mean of all samples so far,
 *   (float)(((double)sum 2^-32 + side) (pixel_samples_scale / passes)),
 * NaN / +-Inf where a sample was, as rt_render gives them; one pass resolves to rt_render's
 * image of that seed bit for bit (while no sample overflowed in either), no pass to zeros.
 * var [rows][W]: the variance of the mean luminance, M2 / ((passes - 1) passes), from
 * Welford's recurrence over the passes' luminance (0.2126 r + 0.7152 g + 0.0722 b of each
 * pass's own mean image, in fp64); 0 before the second pass.  Rows as rt_render's.  Either
 * pointer may be NULL.  _device: pointers on the accumulator's device; both forms return
 * after the work completes. */
int rt_accum_resolve(rt_accum* a, float* rgb_host, float* var_host);
int rt_accum_resolve_device(rt_accum* a, float* rgb_dev, float* var_dev);

typedef struct {
  int32_t passes, max_passes;
  uint64_t samples_per_pixel;  /* spp_sqrt^2 * passes */
  uint64_t nonfinite_pixels;   /* pixels whose variance or mean luminance is not finite */
  /* over the other pixels: sqrt(mean(var)), mean(luminance), and the first over the second
   * (+ 1e-6).  A fixed-order fp64 reduction on the device: the same passes in the same order
   * give the same bits. */
  double rms_std_error, mean_luminance, rel_error;
} rt_accum_info;
int rt_accum_info_get(rt_accum* a, rt_accum_info* out);

/* Adaptive passes (DESIGN.md "Adaptive passes"): a pass over the noisy tiles only.  Added
 * without an ABI version change: detect by the symbols.
 *
 * A tile is a tile x tile block of the share's local image (local row, column; edge tiles are
 * smaller).  Over the pixels of tile T whose variance (as rt_accum_resolve's var) and mean
 * luminance are finite, summed in a fixed order in fp64,
 *   e_T = sqrt(mean var_p) / (max(mean mean_p, 0) + lum_floor),    0 without such a pixel,
 * rounded to fp32.  T is active when some pixel of it has taken fewer than min_passes passes or
 * e_T > rel_error; a pixel is active when its tile is.  lum_floor's default keeps dark tiles
 * from dominating: a linear luminance of 1e-2 is 25/256 after the image writer's sqrt (a
 * choice, not a measurement).  Selecting on the samples' own variance biases the estimate, as
 * in every adaptive sampler; min_passes and tile-level decisions are the mitigation. */
typedef struct {
  double rel_error;    /* tile threshold; must be > 0 */
  double lum_floor;    /* 0 -> 1e-2 */
  int32_t tile;        /* 0 -> 8; 1..64 */
  int32_t min_passes;  /* 0 -> 4; >= 2 */
} rt_adapt_opts;

/* The selection: the active pixels in ascending local index, built on the device by a
 * deterministic compaction (the same state gives the same selection); their number comes back
 * in *n_active_pixels (may be NULL).  rt_accum_select chooses by the tile rule above,
 * rt_accum_set_active takes the caller's mask ([rows][W] bytes, nonzero = active).  The
 * options and the mask pointer are checked before the accumulator and before any device is
 * touched (RT_ERR_INVALID). */
int rt_accum_select(rt_accum* a, const rt_adapt_opts* opts, uint64_t* n_active_pixels);
int rt_accum_set_active(rt_accum* a, const uint8_t* mask_host, uint64_t* n_active_pixels);
/* One pass over the current selection: every active pixel gets exactly the samples a whole
 * pass of `seed` gives it (the random stream is keyed by seed, pixel and sample; the sums are
 * integers), the others are left alone; stats->samples = active pixels * spp_sqrt^2.  It
 * counts one pass against max_passes like rt_accum_add.  RT_ERR_INVALID when no selection was
 * made since the last pass or reset: a selection is consumed by one pass.  An empty selection
 * is a no-op that counts no pass; a selection of every pixel takes rt_accum_add's path.
 * RT_ERR_UNSUPPORTED, with the state unchanged, for an accumulator of RT_MODE_WAVEFRONT and
 * for a scene structure chosen by a tuning knob (RT_TREE=2, RT_BVH8) that has no active-pixel
 * kernel.  (A scene whose whole passes traverse the BVH2 without RT_TREE asking for
 * it traverses the BVH4 of the same leaf records in an active pass.)  An active pass never
 * allocates: it writes chunk records when its chunks fit the buffer the whole passes left, and
 * adds to the pixels with atomics otherwise (the same integers; stats->chunk_records = 0).  From the first such pass on, rt_accum_resolve divides every pixel's sums by the
 * pixel's own pass count and var is M2 / ((n - 1) n) with it (a pixel that took every pass
 * resolves to the same bits as before); rt_accum_info.passes counts the calls that rendered,
 * samples_per_pixel is the most any pixel has.  rt_accum_reset returns to whole passes. */
int rt_accum_add_active(rt_accum* a, uint64_t seed, rt_stats* stats);
/* passes per pixel, [rows][W]; _device: a pointer on the accumulator's device */
int rt_accum_counts(rt_accum* a, int32_t* counts_host);
int rt_accum_counts_device(rt_accum* a, int32_t* counts_dev);
/* e_T of every tile, [tiles_y][tiles_x], as rt_accum_select computes and compares it (opts'
 * rel_error is checked, not used).  err_host NULL: the sizes only. */
int rt_accum_tile_error(rt_accum* a, const rt_adapt_opts* opts, float* err_host, int32_t* tiles_x,
                        int32_t* tiles_y);

typedef struct {
  uint64_t active_pixels;  /* of the last selection */
  uint64_t total_samples;  /* spp_sqrt^2 * the sum of the pass counts */
  int32_t min_count, max_count;
  int32_t n_tiles, active_tiles;  /* of the last rt_accum_select (0 after rt_accum_set_active) */
} rt_adapt_info;
int rt_accum_adapt_info(rt_accum* a, rt_adapt_info* out);

/* Accumulator-owned feature buffers (DESIGN.md "Accumulator-owned feature buffers"): the
 * feature sums of exactly the camera samples the accumulator's passes rendered, kept per pixel
 * on the device next to the image sums.  Added without an ABI version change: detect by the
 * symbols.
 *
 * rt_accum_set_features chooses the plane groups (a mask of RT_ACCUM_FEAT_*; 0 frees them): only
 * while the accumulator holds no pass (else RT_ERR_INVALID, as for unknown bits).  The planes
 * are a second allocation of 56 (guides) + 52 (emit) bytes per pixel of the share plus 56 of
 * staging; RT_ERR_OOM leaves the features off.  With features on, every rt_accum_add /
 * rt_accum_add_active also casts, for the same seed and the same pixels and on the same stream,
 * the feature rays of ALL spp_sqrt^2 samples (the rays, the hit evaluation and L_j of
 * rt_render_aov_emit), sums them per pass in fp32 in sample order as rt_render_aov does and adds
 * the pass's sums to fp64 sums (the light-sample count to an exact integer).  The image sums,
 * the variance and the pass's rt_stats are not affected; the pass is counted only when both were
 * enqueued.  rt_accum_reset clears the feature sums and keeps the setting.
 *
 * rt_accum_resolve_aov writes, for a pixel that took n passes (N = n spp_sqrt^2 samples), every
 * plane as (float)(sum / N) with the division in fp64, coverage = (float)(light samples / N), and
 * zeros where n = 0: one pass of seed s gives rt_render_aov_emit(n_samples = spp_sqrt^2, seed s)
 * to within the rounding of that call's reciprocal (bit-equal when spp_sqrt^2 is a power of two;
 * coverage always).  Any pointer may be NULL, emit may be NULL; RT_ERR_INVALID when a group is
 * asked for that is not enabled, when out->material is not NULL (no material plane is kept:
 * "the kind of sample 0" has no meaning over several passes) or when no buffer is wanted.
 * _device: pointers on the accumulator's device; both forms return after the work completes.
 *
 * RT_ACCUM_FEAT_MEDIA modifies GUIDES / EMIT (alone it is RT_ERR_INVALID): the feature rays are
 * rt_render_aov_media's, so the groups' sums become first-event sums, and the scatter samples of
 * every pixel are counted into an exact integer, 4 more bytes per pixel and 4 of staging.
 * rt_accum_resolve_aov on such an accumulator returns the first-event planes.
 * rt_accum_resolve_aov_media is rt_accum_resolve_aov with the scatter plane,
 * scatter = (float)(scatter samples / N) as coverage; media must not be NULL, media->scatter may
 * be; asking for scatter on an accumulator without the bit is RT_ERR_INVALID, and so is a call
 * that wants no buffer.  One pass of seed s gives rt_render_aov_media(n_samples = spp_sqrt^2,
 * seed s) as above; scatter always exactly. */
#define RT_ACCUM_FEAT_GUIDES 1u   /* albedo, normal, depth */
#define RT_ACCUM_FEAT_EMIT   2u   /* emission, surface_albedo, coverage */
#define RT_ACCUM_FEAT_MEDIA  4u   /* modifies GUIDES / EMIT: their sums become first-event sums, and a
                                     scatter count (an exact integer) is kept per pixel */
int rt_accum_set_features(rt_accum* a, uint32_t planes);
int rt_accum_get_features(rt_accum* a, uint32_t* planes);
int rt_accum_resolve_aov(rt_accum* a, const rt_aov* out_host, const rt_aov_emit* emit_host);
int rt_accum_resolve_aov_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_emit* emit_dev);
int rt_accum_resolve_aov_media(rt_accum* a, const rt_aov* out_host, const rt_aov_emit* emit_host,
                               const rt_aov_media* media_host);
int rt_accum_resolve_aov_media_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_emit* emit_dev,
                                      const rt_aov_media* media_dev);

/* Accumulator-owned chain sums (DESIGN.md "Temporal history for mirrors"): the planes of
 * rt_render_aov_spec for exactly the camera samples the passes rendered, which rt_reproject_spec
 * consumes.  Added without an ABI version change: detect by the symbols.
 * RT_ACCUM_FEAT_SPEC is a plane group of its own that goes with GUIDES and/or EMIT: alone it is
 * RT_ERR_INVALID, and so it is together with MEDIA (a chain traces no media).
 * rt_accum_set_features_spec is rt_accum_set_features with the chain limits, and the one entry
 * that takes the bit: spec_opts NULL means rt_render_aov_spec's defaults, with that entry's range
 * checks (RT_ERR_INVALID for max_bounces < 0 or > 64, a negative or non-finite max_fuzz).
 * rt_accum_set_features itself is unchanged: to it 8 stays an unknown bit, RT_ERR_INVALID, as every
 * caller of it has seen so far; rt_accum_get_features reports the bit.  The same rules: only while the accumulator holds no pass; RT_ERR_OOM leaves the
 * features off.  The group is 40 more bytes per pixel of the share (three fp64 normal sums, one
 * fp64 depth sum, one 64-bit count of specular vertices) and 20 of staging; no albedo is kept.
 * With the bit on, every rt_accum_add / rt_accum_add_active also runs, on the same stream for the
 * same seed and pixels, the chain fold: rt_render_aov_spec's samples for ALL spp_sqrt^2 samples,
 * summed per pass in fp32 in sample order, the pass's normal and depth sums added to the fp64
 * planes and its specular vertices to the exact count.  The first hit is traced twice, once by the
 * GUIDES / EMIT fold and once by the chain fold; an accumulator without the bit launches and
 * allocates exactly what it did.
 * rt_accum_resolve_aov_spec writes out->normal and out->depth as (float)(sum / N) with the division
 * in fp64 and spec->bounces as (float)((double)vertices / N), zeros where n = 0.  RT_ERR_INVALID
 * when out->albedo or out->material is not NULL, when the group is not enabled, or when no buffer
 * is wanted.  One pass of seed s gives rt_render_aov_spec(n_samples = spp_sqrt^2, seed s) in normal
 * and depth to within the rounding of that call's reciprocal (bit-equal when spp_sqrt^2 is a power
 * of two); bounces always exactly, so a pixel all of whose samples passed k vertices resolves to
 * exactly (float)k over any number of passes. */
#define RT_ACCUM_FEAT_SPEC   8u   /* the specular chains' normal, depth and bounces; with GUIDES / EMIT, not MEDIA */
int rt_accum_set_features_spec(rt_accum* a, uint32_t planes, const rt_aov_spec_opts* spec_opts);
int rt_accum_resolve_aov_spec(rt_accum* a, const rt_aov* out_host, const rt_aov_spec* spec_host);
int rt_accum_resolve_aov_spec_device(rt_accum* a, const rt_aov* out_dev, const rt_aov_spec* spec_dev);

/* ------------------------------------------------------------------------ */
/* Temporal reprojection (DESIGN.md "Temporal reprojection"): the previous   */
/* frame's colour, variance and history length carried into a new camera     */
/* through the depth and normal buffers, the stage Schied et al.,            */
/* "Spatiotemporal Variance-Guided Filtering", HPG 2017, put in front of the */
/* spatial filter.  A pure image operation: no scene (which is static: there */
/* are no motion vectors).  Added without an ABI version change: detect by   */
/* the symbols.                                                              */
/* ------------------------------------------------------------------------ */
typedef struct {            /* one frame on one device (or host), whole image, row-major */
  float* rgb;               /* [h][w][3] linear mean colour */
  float* var;               /* [h][w]    variance of the mean luminance (rt_accum_resolve's); NULL = 0 */
  float* count;             /* [h][w]    history weight n of the pixel; NULL = count_scalar everywhere */
  float* normal;            /* [h][w][3] rt_aov's normal */
  float* depth;             /* [h][w]    rt_aov's depth */
  float  count_scalar;      /* used when count is NULL (e.g. the accumulator's passes) */
  int32_t _pad;
} rt_frame;

typedef struct {
  float max_history;        /* 0 -> 8 x the current pixel's count; cap on the reprojected weight */
  float depth_tol;          /* 0 -> 0.05 (relative) */
  float normal_tol;         /* 0 -> 0.1  (|n_p - n_q|^2) */
  float min_weight;         /* 0 -> 0.01 (sum of the valid bilinear weights) */
} rt_reproject_opts;

/* out = the frame `cur` (seen by cam_cur) blended with the history `prev` (seen by cam_prev)
 * found behind each of its pixels.  out uses rgb, var and count; each may be NULL = not wanted,
 * but at least one is required; its normal and depth are not written (the current frame's are
 * the new history's).  opts NULL: the defaults.
 *
 * Per pixel p = (x, y) of the current frame.  The host derives both cameras in fp64
 * (rt_camera_derive) and hands the kernel fp32 vectors relative to a camera's centre, every
 * difference of positions taken in fp64 before the rounding: with C, P00, U, V a camera's
 * center, pixel00, delta_u, delta_v (suffix c: cam_cur, p: cam_prev) these are D = Cc - Cp,
 * Ac = P00c - Cc, Uc, Vc, Ap = P00p - Cp, Up, Vp.  The kernel works in fp32.
 *   current pixel valid: the three colour channels and var are finite, and n_c = count is
 *     finite and > 0.  If not, out takes the current pixel's rgb, var and count bit for bit.
 *   history lookup: there is NO HISTORY when depth_cur(p) is not finite or <= 0 (a miss), or
 *     when normal_cur(p) is not finite.  Otherwise
 *       dir = Ac + x Uc + y Vc,   r = D + depth_cur(p) dir / |dir|   (the hit point relative to
 *       the previous centre),   d' = |r|,
 *       Wp = Up x Vp,  num = Ap . Wp,  den = r . Wp,  s = num / den;
 *     no history unless s is finite and > 0 (the point lies in front of the previous camera);
 *       q = s r - Ap,   u = q . Up / Up . Up,   v = q . Vp / Vp . Vp
 *     (integer (u, v) are pixel centres), x0 = floor(u), y0 = floor(v), and the four taps
 *     (x0 + a, y0 + b), a, b in {0, 1}, have the bilinear weights
 *     beta = (a ? u - x0 : 1 - (u - x0)) (b ? v - y0 : 1 - (v - y0)).
 *   tap valid: it is inside the image; the previous rgb and var are finite; n_q is finite and
 *     > 0; depth_q > 0; |depth_q - d'| <= depth_tol d'; |n_p - n_q|^2 <= normal_tol.
 *     S = sum of beta over the valid taps.  If S < min_weight there is no history.
 *   reprojected history: c_h = sum beta c_q / S,  v_h = sum beta^2 v_q / S^2 (the taps as
 *     independent estimators, the rule rt_denoise_var applies to its taps),
 *     n_h = min(sum beta n_q / S, max_history).
 *   blend: out.rgb = (n_h c_h + n_c c) / (n_h + n_c),
 *     out.var = (n_h^2 v_h + n_c^2 v) / (n_h + n_c)^2,  out.count = n_h + n_c.
 *     With no history n_h = 0 and out is the current pixel's bits.
 * Argument checks, before any device is touched.  RT_ERR_INVALID: a NULL camera, frame or out;
 * a missing rgb, normal or depth in prev or cur; out without any buffer; w or h <= 0 (or
 * w h >= 2^31 / 3), or a camera whose derived width / height is not w x h; negative or
 * non-finite options; any out buffer that is also a prev buffer (the taps gather from prev, so
 * prev cannot be written; out may alias cur).  RT_ERR_UNSUPPORTED: either camera has
 * defocus_angle > 0 (depth is then measured from the lens sample, not from the centre).
 * rt_reproject: host pointers, staged through the device (device 0); rt_reproject_device: device
 * pointers on `device`, enqueued on `stream` (hipStream_t or NULL), returns after the work
 * completes.  Two calls give identical bits. */
int rt_reproject(const rt_camera* cam_prev, const rt_frame* prev, const rt_camera* cam_cur,
                 const rt_frame* cur, int w, int h, const rt_reproject_opts* opts,
                 const rt_frame* out);
int rt_reproject_device(const rt_camera* cam_prev, const rt_frame* prev_dev,
                        const rt_camera* cam_cur, const rt_frame* cur_dev, int w, int h,
                        const rt_reproject_opts* opts, const rt_frame* out_dev, int device,
                        void* stream);

/* rt_reproject with the directly seen emission kept out of the history (DESIGN.md "Temporal
 * reprojection"; the emission split of rt_denoise_emit applied to the temporal stage): a light
 * that lies in a surface's plane passes the depth and normal tests, and without the split the
 * bilinear taps bleed it into the pixels beside it, frame after frame.  Added without an ABI
 * version change (rt_frame and rt_reproject_opts are unchanged): detect by the symbols.
 * prev_emit / cur_emit: the frames' rt_aov_emit (rt_accum_resolve_aov's of an accumulator with
 * RT_ACCUM_FEAT_EMIT); emission and coverage are required, surface_albedo is not read and may be
 * NULL.  The definition is rt_reproject's with exactly these changes.  Per frame and pixel let
 *   k = 1 - coverage,   z = (rgb - emission) / k   (the surface radiance per sample that saw no
 *   light),   v_z = var / k^2;   the history weight n stays in pixel units.
 *   current pixel valid: the parent's rule, and emission finite, and coverage finite with
 *     0 <= coverage < 1.
 *   tap valid: the parent's rule, and the tap's emission finite and 0 <= coverage_q < 1.  A fully
 *     covered pixel carries no surface information: it is never a tap and never takes history.
 *   reprojected history and blend: the parent's formulas for c_h, v_h, n_h, the cap and the
 *     blend, applied to z, v_z and n (z_q, v_z_q of the taps; z_c, v_z_c of the current pixel).
 *   output, pixels that found history: out.rgb = k_c z_blend + emission_c, out.var = k_c^2
 *     v_blend, out.count = n_h + n_c: the emission is deterministic and adds no variance.
 *   output, every other pixel (invalid, a miss, coverage 1, S < min_weight): rgb, var and count
 *     pass through bit for bit, also when out aliases cur.
 * The operations run in this order: subtract, divide, then multiply-add; so with emission = 0 and
 * coverage = 0 in both frames the result is rt_reproject's bit for bit.
 * Argument checks, before any device is touched: the parent's, and RT_ERR_INVALID for a NULL
 * prev_emit or cur_emit, for a missing emission or coverage in either, and for an out buffer that
 * is also a buffer of prev_emit.  out may alias cur's and cur_emit's buffers (the current pixel
 * is read whole before any write).  Host and device forms as rt_reproject's; rt_reproject_emit
 * stages 104 bytes per pixel.  Two calls give identical bits. */
int rt_reproject_emit(const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                      const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit,
                      int w, int h, const rt_reproject_opts* opts, const rt_frame* out);
int rt_reproject_emit_device(const rt_camera* cam_prev, const rt_frame* prev_dev,
                             const rt_aov_emit* prev_emit_dev, const rt_camera* cam_cur,
                             const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev, int w, int h,
                             const rt_reproject_opts* opts, const rt_frame* out_dev, int device,
                             void* stream);

/* rt_reproject_emit with emission and coverage carried as history planes of their own (DESIGN.md
 * "Light history").  rt_reproject_emit re-lights a pixel with the current frame's emission and
 * coverage, so on the rim of a light, where coverage is a fraction estimated from a few samples, no
 * history improves the pixel.  Here both planes are reprojected and blended with the weights of the
 * surface radiance, and the pixel is re-lit from the blend.  Added without an ABI version change:
 * detect by the symbols.  out_emit: the new history's light planes, emission and coverage; either
 * may be NULL = not wanted; surface_albedo is never read or written.
 * The definition is rt_reproject_emit's with exactly these changes.  Per frame and pixel let
 * kappa = coverage, E = emission, z = (rgb - E) / (1 - kappa), v_z = var / (1 - kappa)^2.
 *   current pixel valid: rgb and var finite, n_c finite and > 0, E_c finite, 0 <= kappa_c <= 1: a
 *     fully covered pixel is valid.  It has no surface sample: its weight in the surface blend is
 *     w_c = 0 and the divisor of its z_c and v_z,c is taken as 1; otherwise w_c = n_c.  An invalid
 *     pixel passes through: out takes its rgb, var and count, out_emit its emission and coverage,
 *     bit for bit.
 *   history lookup: rt_reproject's (depth, normal, s, the four taps and their beta).
 *   light tap: rt_reproject's tap rule (inside the image, rgb_q and var_q finite, n_q finite and
 *     > 0, depth_q > 0, the depth and normal tolerances), and E_q finite and 0 <= kappa_q <= 1.
 *   surface tap: a light tap with kappa_q < 1: exactly rt_reproject_emit's tap.  A fully covered
 *     previous pixel is a light tap and not a surface tap.
 *   An invalid tap's values are selected to 0 (its divisor to 1) before any arithmetic.
 *   surface history, over the surface taps: S_z = sum beta, z_h = sum beta z_q / S_z, v_h = sum
 *     beta^2 v_z,q / S_z^2, n_h = min(sum beta n_q / S_z, cap), cap = max_history or 8 n_c;
 *     n_h = 0 when S_z < min_weight.
 *   light history, over the light taps: S_l = sum beta, E_h = sum beta E_q / S_l, kappa_h = sum
 *     beta kappa_q / S_l, m_h = min(sum beta n_q / S_l, cap); m_h = 0 when S_l < min_weight.
 *   pass-through, all five planes bit for bit: n_h = 0 and m_h = 0 (no history); or n_h + w_c = 0
 *     (covered now and no surface history: the inside of a light).
 *   blend, every other pixel:
 *     z_blend = (n_h z_h + w_c z_c) / (n_h + w_c),
 *     v_blend = (n_h^2 v_h + w_c^2 v_z,c) / (n_h + w_c)^2,
 *     kappa_out = (m_h kappa_h + n_c kappa_c) / (m_h + n_c),
 *     E_out = (m_h E_h + n_c E_c) / (m_h + n_c),
 *     out.rgb = (1 - kappa_out) z_blend + E_out,   out.var = (1 - kappa_out)^2 v_blend,
 *     out.count = max(n_h, m_h) + n_c,   out_emit = E_out, kappa_out.
 *   out.var is rt_reproject_emit's rule: the light adds no variance.  Where coverage is a
 *   fraction (a rim) the blended coverage is itself an estimate whose variance is not counted:
 *   out.var is knowingly too small there.
 * The operations run in rt_reproject_emit's order: subtract, divide, then multiply-add.  With
 * emission = 0 and coverage = 0 in both frames every light tap is a surface tap, m_h = n_h, and
 * rgb, var and count are rt_reproject's bit for bit; out_emit is all zero.
 * Argument checks, before any device is touched: rt_reproject_emit's, and RT_ERR_INVALID for a
 * NULL out_emit and for an out_emit emission or coverage that is a buffer of prev or prev_emit.
 * out and out_emit may alias cur's and cur_emit's buffers (the current pixel is read whole before
 * any write).  Host and device forms as rt_reproject's; rt_reproject_light stages 104 bytes per
 * pixel.  Two calls give identical bits. */
int rt_reproject_light(const rt_camera* cam_prev, const rt_frame* prev, const rt_aov_emit* prev_emit,
                       const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit,
                       int w, int h, const rt_reproject_opts* opts, const rt_frame* out,
                       const rt_aov_emit* out_emit);
int rt_reproject_light_device(const rt_camera* cam_prev, const rt_frame* prev_dev,
                              const rt_aov_emit* prev_emit_dev, const rt_camera* cam_cur,
                              const rt_frame* cur_dev, const rt_aov_emit* cur_emit_dev, int w, int h,
                              const rt_reproject_opts* opts, const rt_frame* out_dev,
                              const rt_aov_emit* out_emit_dev, int device, void* stream);

/* The three reprojections above with the second raw moment of luminance carried as one more
 * history plane, and the variance taken from the moments (DESIGN.md "Luminance moments"; Schied et
 * al.'s temporal and spatial variance estimates).  The accumulator's variance is an estimate
 * across the passes of one frame: 0 for a frame of one pass, however long its history.  Here the
 * variance comes from the history itself once it is long enough, and below that from a window of
 * the current frame, so frames of one pass can be filtered by rt_denoise_var.  Added without an
 * ABI version change: detect by the symbols.
 * mode selects the definition this one is a delta on: RT_REPROJECT_PLAIN rt_reproject's (prev_emit,
 * cur_emit and out_emit are not read), RT_REPROJECT_EMIT rt_reproject_emit's (out_emit is not read),
 * RT_REPROJECT_LIGHT rt_reproject_light's.  prev_lum2 and out_lum2 are [h][w] float planes; mopts
 * NULL: the defaults.  Call x the colour the mode carries and blends: rgb in PLAIN, z = (rgb - E) /
 * (1 - kappa) in EMIT and LIGHT exactly as those modes form it; w_c the weight of the current x
 * in the blend: n_c in PLAIN and EMIT, rt_reproject_light's w_c in LIGHT; Y the luminance of
 * rt_denoise_var, evaluated in fp32 as (0.2126 r + 0.7152 g) + 0.0722 b.
 * The first raw moment needs no plane: Y is linear and the moment is blended by the weights the
 * colour is blended with, so it is Y of the blended colour.
 * Everything not named here is the selected mode's definition: the history lookup, tap validity,
 * S, the cap, c_h, n_h, the blends of colour, count, emission and coverage, the pass-through sets.
 *   current pixel: y_c = Y(x_c), q_c = y_c^2.
 *   tap valid: the mode's rule (in LIGHT: the light tap's, so the surface tap's too), and the tap's
 *     lum2 finite.  An invalid tap's lum2 is selected to 0 before any arithmetic.
 *   history: q_h = sum beta q_tap / S over the taps of the surface colour.
 *   blend: q_out = (n_h q_h + w_c q_c) / (n_h + w_c),   y_out = Y(x_blend).
 *   history length in frames: K = (n_h + w_c) / w_c, for a pixel with surface history and w_c > 0.
 *   temporal estimate: v_t = max(q_out - y_out^2, 0) / (K - 1): the variance of the blended mean
 *     when K equally weighted frames are independent.  Exact while the cap has not bitten;
 *     knowingly approximate once it has (old frames then weigh less than K says), or when the
 *     frames bring different counts.
 *   spatial estimate (radius >= 0): over the pixels t of the CURRENT frame with |t - p| <= radius
 *     in both coordinates that are inside the image, valid by the mode's current-pixel rule with
 *     kappa_t < 1 where the mode has a coverage, and within |depth_t - depth_p| <= depth_tol
 *     depth_p and |n_p - n_t|^2 <= normal_tol (rt_reproject_opts'; p itself always counts).  T is
 *     their number, a = sum Y(x_t) / T, b = sum Y(x_t)^2 / T, an unweighted box summed in fp32 row
 *     by row in ascending order;  v_s = max(b - a^2, 0) (T / (T - 1)) / K, and 0 when T < 2.  It
 *     counts texture detail inside the window as noise, as SVGF's spatial estimate does.
 *   the variance v the mode carries on in place of its v_blend, for a pixel with w_c > 0:
 *     v_t when the pixel found surface history and K >= min_frames; otherwise v_s, with K = 1 for
 *     a pixel without surface history.  radius = -1: the mode's v_blend, unchanged (and the
 *     current pixel's var where the mode passes it through).  A pixel of LIGHT with w_c = 0 that
 *     blends (covered now, surface history behind it) keeps the mode's v_blend, and q_out = q_h.
 *   re-lighting: what the mode does to v_blend is unchanged: out.var = k_c^2 v in EMIT,
 *     (1 - kappa_out)^2 v in LIGHT, v in PLAIN.
 *   pixels without surface history that are valid by the mode's rule with w_c > 0: rgb, count (and
 *     LIGHT's blend of emission and coverage, where it has light history) as the mode writes them,
 *     out_lum2 = q_c, out.var = the re-lit v_s (K = 1): k_c^2 v_s where the mode passes the pixel
 *     through.  The one departure from "passes through bit for bit"; none with radius = -1.
 *   invalid pixels, and covered pixels without surface history (LIGHT's inside of a light, EMIT's
 *     kappa = 1): every plane passes through as the mode does, out_lum2 = 0.  Never taps.
 *   no history at all: prev == NULL (cam_prev, prev_emit and prev_lum2 are then not read): every
 *     pixel takes the no-history path, which is also what a prev of zero counts gives.  This makes
 *     the first frame of a sequence filterable.
 * Order of operations, in fp32: q of every frame is formed before the blend (q_c = y_c y_c; the
 * taps bring theirs); q_out as written, a sum of two products times 1 / (n_h + w_c); then the
 * subtraction q_out - y_out y_out, which cancels against y^2 and not against the variance: its
 * rounding error is a few 2^-24 of lum2, whatever the variance.
 * Argument checks, before any device is touched: the selected mode's own; RT_ERR_INVALID for an
 * unknown mode; a NULL out_lum2; a prev given without prev_lum2; radius < -1 or > 8; min_frames
 * negative, not finite or in (0, 2) (it would divide by K - 1 <= 0); out_lum2 equal to any input
 * plane (of prev, prev_emit, prev_lum2, cur or cur_emit) or to an out or out_emit buffer; an out or
 * out_emit buffer equal to prev_lum2 (a plane the taps gather, like prev's); and ANY out or out_emit
 * buffer that is a buffer of cur or cur_emit: the window reads the current frame's neighbours, so the "out may
 * alias cur" of the older entries cannot hold here.  Host and device forms as rt_reproject's;
 * rt_reproject_moments stages 100 bytes per pixel in PLAIN, 132 in EMIT and 148 in LIGHT.  Two
 * calls give identical bits. */
enum { RT_REPROJECT_PLAIN = 0, RT_REPROJECT_EMIT = 1, RT_REPROJECT_LIGHT = 2 };
typedef struct {
  float   min_frames;       /* 0 -> 4: the history length, in frames, from which the moments are trusted */
  int32_t radius;           /* 0 -> 3 (a 7 x 7 window); -1: no spatial estimate; at most 8 */
} rt_moments_opts;
int rt_reproject_moments(int mode, const rt_camera* cam_prev, const rt_frame* prev,
                         const rt_aov_emit* prev_emit, const float* prev_lum2,
                         const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit,
                         int w, int h, const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                         const rt_frame* out, const rt_aov_emit* out_emit, float* out_lum2);
int rt_reproject_moments_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                                const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev,
                                const rt_camera* cam_cur, const rt_frame* cur_dev,
                                const rt_aov_emit* cur_emit_dev, int w, int h,
                                const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                                const rt_frame* out_dev, const rt_aov_emit* out_emit_dev,
                                float* out_lum2_dev, int device, void* stream);

/* rt_reproject_moments with the history colour rectified before the blend: variance clipping
 * (Salvi, "An excursion in temporal supersampling", GDC 2016; DESIGN.md "Clamping the history").
 * The history is accepted on the first hit's depth and normal alone; on a mirror or behind glass
 * these agree from frame to frame while the reflection moves under them.  Here the reprojected
 * colour is clamped per channel to mean +- gamma sigma of the current frame's gated neighbourhood,
 * so a history the current frame contradicts is overruled.  Added without an ABI version change:
 * detect by the symbols.  copts follows mopts; copts == NULL is OFF: rt_reproject_moments' result bit
 * for bit in every plane.  With copts given, everything not named here is rt_reproject_moments'
 * definition in the selected mode (x, w_c, Y as there).
 *   window: the spatial estimate's, with the same mopts.radius: the pixels t of the current frame
 *     with |t - p| <= radius in both coordinates that are inside the image, valid by the mode's
 *     current-pixel rule with kappa_t < 1 where the mode has a coverage, and within depth_tol and
 *     normal_tol of p (p itself always counts).  T is their number.
 *   shifted sums, per channel j: d_t,j = x_t,j - x_p,j, x_p the current pixel's colour;
 *     A_j = sum d_t,j, B_j = sum d_t,j^2, in fp32 row by row in ascending order; an excluded
 *     pixel's d is selected to 0 before any arithmetic.
 *   box: m_j = x_p,j + A_j / T,   s_j = sqrt(max(B_j / T - (A_j / T)^2, 0)).  The deviations are
 *     taken from x_p so that a noise-free neighbourhood gives s = 0 exactly, and so that the
 *     subtraction cancels against the spread and not against the magnitude.
 *   clamp, for a pixel with surface history, w_c > 0 and T >= 2:
 *     x_h'_j = min(max(x_h,j, m_j - gamma s_j), m_j + gamma s_j);  x_h' stands in for the mode's
 *     history colour c_h in the blend and so in y_out = Y(x_blend).  Nothing else changes: n_h,
 *     v_h, q_h, the cap, LIGHT's emission and coverage history are rt_reproject_moments'.
 *     q_h is NOT rectified: a clamped pixel's y_out moves away from the mean its moments were
 *     collected around, so its v_t = max(q_out - y_out^2, 0) / (K - 1) is no longer the variance
 *     of its mean.  Where the clamp lowers the history's luminance (a bright stale history over a
 *     darker frame) y_out^2 falls and v_t can only grow.  That is intended: a pixel whose history
 *     was overruled is filtered harder.  Where the clamp raises it (a dark stale history over a
 *     brighter frame) v_t shrinks, at the least to 0, and the filter leaves the pixel more alone.
 *   not clamped, rt_reproject_moments' bits: pixels without surface history, pixels with T < 2,
 *     LIGHT's pixels with w_c = 0, every pass-through set.
 * The previous frame's values reach the clamp as the taps' sums, formed from selected values only:
 * a NaN of the previous frame never meets arithmetic here either.
 * Argument checks, before any device is touched: rt_reproject_moments' own; RT_ERR_INVALID for
 * copts given with mopts.radius resolving to -1 (there is no window); gamma negative or not finite.
 * Host and device forms as rt_reproject_moments'; rt_reproject_clip stages what it stages; the
 * device entry allocates nothing.  Two calls give identical bits. */
typedef struct {
  float   gamma;            /* 0 -> 0.75 (DESIGN.md section 22's sweep): the box is mean +- gamma * sigma per channel */
} rt_clip_opts;
int rt_reproject_clip(int mode, const rt_camera* cam_prev, const rt_frame* prev,
                      const rt_aov_emit* prev_emit, const float* prev_lum2,
                      const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit,
                      int w, int h, const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                      const rt_clip_opts* copts, const rt_frame* out, const rt_aov_emit* out_emit,
                      float* out_lum2);
int rt_reproject_clip_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                             const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev,
                             const rt_camera* cam_cur, const rt_frame* cur_dev,
                             const rt_aov_emit* cur_emit_dev, int w, int h,
                             const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                             const rt_clip_opts* copts, const rt_frame* out_dev,
                             const rt_aov_emit* out_emit_dev, float* out_lum2_dev, int device,
                             void* stream);

/* rt_reproject_clip with the history of a mirror looked up through the virtual point (DESIGN.md
 * "Temporal history for mirrors").  Added without an ABI version change: detect by the symbols.
 * For a planar perfect mirror, C + D d^ (C the camera centre, d^ the unit camera ray, D the depth
 * summed along the specular chain) is the mirror image of the chain's terminal vertex, and any
 * other camera sees that vertex, through the mirror, at exactly its distance to that point.  So
 * the whole history lookup of rt_reproject is kept, formula for formula (r = D + depth dir/|dir|,
 * d' = |r|, the projection, the depth and normal tests against the tap), and is FED the chain's
 * planes: the entry does not know what `normal` and `depth` hold.  The caller passes, for both
 * frames, rt_accum_resolve_aov_spec's (or rt_render_aov_spec's) normal and depth; for a pixel with
 * bounces == 0 these have the first hit's bits.
 * The arguments are rt_reproject_clip's with one more struct after copts.  copts == NULL stays "no
 * clamp" (rt_reproject_moments' definition).  spec == NULL: rt_reproject_clip's result bit for bit
 * in every plane.  With spec given, the definition is rt_reproject_clip's with two changes:
 *   current pixel: b_c = cur_bounces(p).  b is WHOLE when it is finite, >= 0 and b == floorf(b).
 *     There is no history unless b_c is whole (a pixel whose samples took chains of different
 *     lengths has meaningless mean planes); such a pixel takes the mode's no-history path exactly
 *     as a miss does: v_s with K = 1, out_lum2 = q_c.
 *   tap valid: the mode's rule, and b_q == b_c, an exact float comparison that a NaN fails.  The
 *     tap's bounces value is used in the comparison only, never in arithmetic.  Without it a
 *     mirror pixel's virtual point could accept a directly seen surface that lies at that depth.
 * The window, the spatial estimate and the clip box gate on depth and normal as before.  On frames
 * whose two bounces planes are all zero the result is rt_reproject_clip's bit for bit.
 * RT_ERR_INVALID, before any device is touched: spec without cur_bounces; prev given without
 * prev_bounces; a bounces plane that is an out buffer; then rt_reproject_clip's refusals.  The
 * host entry stages 8 more bytes per pixel.  Two calls give identical bits.
 * Not covered: curved mirrors (the virtual point is exact for planes only; the gates and the
 * optional clip decide), glass whose samples mix reflection and refraction (fractional bounces:
 * the history is dropped, not stale), fuzzy metals above the chain's max_fuzz, media along the
 * chain, the emission split along the chain, moving geometry, defocus cameras. */
typedef struct {
  const float* prev_bounces;  /* [h][w]; required when prev is given */
  const float* cur_bounces;   /* [h][w]; required */
} rt_spec_planes;
int rt_reproject_spec(int mode, const rt_camera* cam_prev, const rt_frame* prev,
                      const rt_aov_emit* prev_emit, const float* prev_lum2,
                      const rt_camera* cam_cur, const rt_frame* cur, const rt_aov_emit* cur_emit,
                      int w, int h, const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                      const rt_clip_opts* copts, const rt_spec_planes* spec, const rt_frame* out,
                      const rt_aov_emit* out_emit, float* out_lum2);
int rt_reproject_spec_device(int mode, const rt_camera* cam_prev, const rt_frame* prev_dev,
                             const rt_aov_emit* prev_emit_dev, const float* prev_lum2_dev,
                             const rt_camera* cam_cur, const rt_frame* cur_dev,
                             const rt_aov_emit* cur_emit_dev, int w, int h,
                             const rt_reproject_opts* opts, const rt_moments_opts* mopts,
                             const rt_clip_opts* copts, const rt_spec_planes* spec_dev,
                             const rt_frame* out_dev, const rt_aov_emit* out_emit_dev,
                             float* out_lum2_dev, int device, void* stream);

/* ------------------------------------------------------------------------ */
/* Frame pipeline (DESIGN.md "Frame pipeline"): an object that owns, on the  */
/* accumulator's device, everything the low-sample pipeline keeps between    */
/* frames, so that a client with no device allocator of its own (C, cgo)     */
/* runs resolve -> reproject -> filter -> PPM without the frame leaving the  */
/* device.  Added without an ABI version change: detect by the symbols.      */
/* ------------------------------------------------------------------------ */
typedef struct rt_pipeline rt_pipeline;

#define RT_PIPE_FILTER_NONE  0   /* the blended frame is the image */
#define RT_PIPE_FILTER_PLAIN 1   /* rt_denoise[_emit]_device */
#define RT_PIPE_FILTER_VAR   2   /* rt_denoise_var[_emit]_device */

typedef struct {            /* 104 bytes, every field 4 bytes wide: no padding */
  int32_t temporal;         /* 0: no history (resolve -> filter only); 1: reproject */
  int32_t mode;             /* RT_REPROJECT_PLAIN | _EMIT | _LIGHT */
  int32_t moments;          /* rt_reproject_moments_device: lum2 carried, the variance from the moments */
  int32_t clip;             /* rt_reproject_clip_device (needs moments and a window) */
  int32_t specular;         /* rt_reproject_spec_device over the accumulator's chain planes (needs moments) */
  rt_reproject_opts reproject;  /* zeros: the entries' defaults */
  rt_moments_opts   mopts;
  rt_clip_opts      copts;  /* read with clip */
  int32_t filter;           /* RT_PIPE_FILTER_* */
  int32_t split_emitters;   /* the filter's _emit entry */
  rt_denoise_opts     dopts;    /* RT_PIPE_FILTER_PLAIN's; zeros: the defaults (demodulate 0) */
  rt_denoise_var_opts vopts;    /* RT_PIPE_FILTER_VAR's */
} rt_pipeline_opts;

typedef struct {            /* 40 bytes */
  int32_t width, height, device;  /* of the buffers held: 0, 0, -1 before the first push */
  int32_t frames;           /* pushes since create / reset / a dropped history */
  int32_t had_history;      /* the last push found a history to reproject */
  int32_t _pad;
  uint64_t device_bytes;    /* held now */
  uint64_t allocations;     /* device allocations made since create */
} rt_pipeline_info;

/* rt_pipeline_push(p, acc) runs, on the accumulator's device and stream, with exactly the
 * aliasing rt.Temporal uses, the sequence a Python caller writes today:
 *   the temporal half (temporal = 1): rt_accum_resolve_device and rt_accum_resolve_aov_device
 *     (with specular: rt_accum_resolve_aov_spec_device for the history's normal, depth and
 *     bounces) of acc, then the reproject entry the flags select with the stored history as prev,
 *     the accumulator's camera (the one rt_accum_create took) as cam_cur and its pass count as
 *     the current frame's count_scalar.  Two history sets are used in turn.  Without moments out
 *     aliases cur, and a first frame is the frame itself with count filled; with moments the
 *     frame is resolved into a third set (no out buffer of those entries may be cur's) and a
 *     first frame goes through the entry with prev = NULL.  temporal = 0: the frame is the
 *     accumulator's resolve, count the pass count.
 *   the filter half: the entry `filter` and `split_emitters` select, over the blended rgb (and
 *     var), guided by the albedo (split: surface_albedo), normal and depth of the FIRST hit
 *     (rt_accum_resolve_aov_device; with specular these have buffers of their own), and in split
 *     mode by the set's emission and coverage: the blended planes in RT_REPROJECT_LIGHT, the
 *     frame's own otherwise.  It writes an image buffer of the object's own, never the history.
 * Every stage is one of the public _device entries, so its definition, its argument checks and
 * its bits are that entry's; the call blocks as they do.  Device memory is allocated on the first
 * push and when the image size or the device changes (the history is then dropped, as after
 * rt_pipeline_reset); once both history sets are warm no call allocates.  Per pixel and set 40
 * bytes (+16 with emission and coverage, +4 lum2, +4 bounces, +12 the image), 16 (+16 in LIGHT)
 * for the moments' third set, and 12..40 of guides plus 12 for rt_pipeline_ppm's text.
 * The object holds no pointer into an accumulator or a scene between calls: destroying the scene
 * first is legal.
 * RT_ERR_INVALID from rt_pipeline_create, before any device is touched: a NULL argument; an unknown
 * mode or filter; clip or specular without moments; clip with mopts.radius == -1; moments, clip,
 * specular or a non-plain mode with temporal = 0; an option the entries refuse (negative or
 * non-finite reproject options and gamma, radius outside -1..8, min_frames in (0, 2), iterations
 * outside 0..8, a negative or NaN sigma).
 * RT_ERR_INVALID from rt_pipeline_push, before anything is written: a NULL argument; an accumulator
 * with no pass, with no features, without RT_ACCUM_FEAT_GUIDES, without RT_ACCUM_FEAT_EMIT when
 * mode != PLAIN or split_emitters is set, without RT_ACCUM_FEAT_SPEC when specular is set, or of a
 * row share (nranks != 1).  RT_ERR_UNSUPPORTED for a defocus camera comes from the reproject entry.
 * A refused or failed push leaves the history and the last image as they were.
 * rt_pipeline_image: the last push's image [h][w][3] in one copy of 12 bytes per pixel.
 * rt_pipeline_ppm: rt_format_ppm_device of it into a device buffer of the object's, then one copy;
 * returns the byte count; out_host NULL or cap 0 asks the size (the text is formatted once per
 * frame); a cap smaller than the size is RT_ERR_INVALID, as rt_format_ppm's.
 * rt_pipeline_planes_device: borrowed device pointers of the last push, valid until the push after
 * the next (or a push at another size or on another device): blended rgb, var, count and the
 * history's normal and depth; light: emission and coverage as the filter took them (NULL without
 * them); lum2 (NULL without moments); image.  Any out pointer may be NULL.
 * The last three return RT_ERR_INVALID before the first successful push. */
int rt_pipeline_create(const rt_pipeline_opts* opts, rt_pipeline** out);   /* touches no device */
int rt_pipeline_destroy(rt_pipeline* p);
int rt_pipeline_reset(rt_pipeline* p);                                      /* a cut: drop the history, keep the buffers */
int rt_pipeline_push(rt_pipeline* p, rt_accum* acc);
int rt_pipeline_image(rt_pipeline* p, float* rgb_host);
int64_t rt_pipeline_ppm(rt_pipeline* p, char* out_host, int64_t cap);
int rt_pipeline_planes_device(rt_pipeline* p, rt_frame* blended, rt_aov_emit* light, float** lum2, float** image);
int rt_pipeline_info_get(rt_pipeline* p, rt_pipeline_info* out);

/* ------------------------------------------------------------------------ */
/* Frame pipeline over row shares: a frame accumulated as n  */
/* row-interleaved shares (rt_accum_create with opts.rank i of opts.nranks   */
/* n, each on any device) pushed into one pipeline.  Added without an ABI    */
/* version change: detect by the symbols.                                    */
/* ------------------------------------------------------------------------ */
/* rt_accum_add_shares does rt_accum_add(accs[i], seed, ...) for every i, one host thread per share,
 * so that shares on different devices render at the same time; each share's state afterwards is
 * bit for bit what n sequential rt_accum_add calls leave.  stats (may be NULL) is the shares'
 * combined as rt_render_multi combines them: counts and rows summed, the kernel times of the
 * slowest share.  When shares fail, the code and message of the one with the lowest index are
 * returned; the other shares keep the pass they took (their pass counts then differ, which
 * rt_pipeline_push_shares refuses: add the missing pass or rt_accum_reset them all).
 * RT_ERR_INVALID before anything runs: accs NULL, n < 1, a NULL element.
 *
 * rt_pipeline_push_shares is rt_pipeline_push for a frame held as n shares; accs[i] must be the
 * accumulator of rank i of n.  Every plane the stages read equals, bit for bit, what a single
 * nranks == 1 accumulator with the same passes would have resolved, so history, image and PPM are
 * those of rt_pipeline_push.  The lead device is accs[0]'s: the pipeline's buffers live there and
 * the stages run on accs[0]'s stream.  Each share resolves, with the _device resolves
 * rt_pipeline_push calls, into a staging block on its own device; the blocks are copied to a gather
 * buffer on the lead device (a peer copy between devices) and one kernel writes the planes where
 * rt_pipeline_push's resolves write them.  The call blocks, and nothing is in flight on a staging
 * buffer when it returns, failed or not.  A pipeline may be fed by either entry from frame to
 * frame; a push at another size or on another lead device starts over, as rt_pipeline_push's does.
 * rt_pipeline_info.device_bytes and allocations include the gather buffer (one allocation per
 * size, share count and device list); the staging blocks on the shares' devices, at most 96 bytes
 * per pixel of a share, are not in the struct.
 * RT_ERR_INVALID, before anything is written: a NULL argument; n < 1; n greater than the image
 * height (an empty share is not supported); a NULL element; the same accumulator twice; accs[i]
 * whose rank is not i or whose nranks is not n; shares that differ in scene, in camera (a byte
 * compare of rt_camera, which holds width, aspect ratio, samples and max_depth), in feature planes
 * or chain limits, or in pass count; a share that fails a test rt_pipeline_push makes of its
 * accumulator (no pass, missing feature groups).  Active-pixel passes (rt_accum_add_active) are
 * what they are to rt_pipeline_push, which makes no test of them: the resolves divide each pixel by
 * its own count and the frame's count is the accumulator's pass count. */
int rt_accum_add_shares(rt_accum* const* accs, int32_t n, uint64_t seed, rt_stats* stats);
int rt_pipeline_push_shares(rt_pipeline* p, rt_accum* const* accs, int32_t n);

/* Demo scenes mirroring main.go (by name or the main.go -S number).
 * names: book1, book2, book3, simple_light, quads, cornell, cornell_smoke, model
 * The camera receives the scene's settings; override fields afterwards. */
int rt_demo_scene(rt_tree* t, const char* name, const char* asset_dir, rt_camera* cam,
                  int* world, int* lights);
int rt_demo_scene_name(int s_number, const char** name_out);
/* The "model" scene's substitute for dragon.obj (absent from the reference) as OBJ
 * text: nu x nv grid of a torus-knot tube (nu, nv <= 0: 2048 x 256 = 1M triangles).
 * Returns the byte count; call with out = NULL to size.  Writing it to
 * <asset_dir>/dragon.obj lets "model" load it from disk like the real mesh. */
int64_t rt_substitute_mesh_obj(int nu, int nv, char* out, int64_t cap);

/* Number of HIP devices visible (0 on a CPU-only host; never aborts). */
int rt_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
