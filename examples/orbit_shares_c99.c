/* orbit_shares_c99.c — orbit_c99.c's moving camera with every frame accumulated as row shares
 * (INTEGRATION.md "A moving camera over several devices"), still with no HIP
 * runtime and no device allocator of its own.
 *
 * The Go scene cornellBox (main.go:278-320) through the constructor calls of cornell_c99.c, then
 * three frames of an orbit about the look-at point.  Each frame is ONE pass of 4 samples per pixel
 * into SHARES accumulators, rank i of SHARES on DEVICES[i], each with the feature planes
 * (RT_ACCUM_FEAT_GUIDES | RT_ACCUM_FEAT_EMIT); rt_accum_add_shares renders the shares side by side and
 * rt_pipeline_push_shares pushes them as one frame into an rt_pipeline in emit mode with luminance
 * moments and the split variance-guided filter, which lives on DEVICES[0].  rt_pipeline_ppm brings back
 * the frame's P3 text, the only bytes that cross the host link: the bytes orbit_c99.c writes.
 *
 *   orbit_shares_c99 W SEED DEGREES PREFIX      writes PREFIX_000.ppm, PREFIX_001.ppm, PREFIX_002.ppm
 *
 * Frame k is seen from the camera turned by k * DEGREES and rendered with seed SEED + k.  DEVICES is
 * {0, 0, 0}: three shares on one device; a machine with more names them here.
 *
 * Build: gcc -std=c99 -pedantic-errors -Wall -Wextra -Werror -I include examples/orbit_shares_c99.c \
 *          -L go_raytracer_amd -lrt_amd -lm -Wl,-rpath,<dir of librt_amd.so>   (tests/test_c_client_shares.py)
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_abi.h"

#define FRAMES 3
#define SHARES 3
static const int32_t DEVICES[SHARES] = {0, 0, 0};

static int must(int rc, const char* what) {
  if (rc < 0) {
    fprintf(stderr, "%s: %d (%s)\n", what, rc, rt_last_error());
    exit(2);
  }
  return rc;
}

static int lambertian(rt_tree* t, double r, double g, double b) { /* NewLambertian materials.go:35 */
  return must(rt_mat_lambertian(t, must(rt_tex_solid(t, r, g, b), "tex")), "lambertian");
}
static int light(rt_tree* t, double r, double g, double b) { /* NewDiffuseLight materials.go:136 */
  return must(rt_mat_diffuse_light(t, must(rt_tex_solid(t, r, g, b), "tex")), "light");
}
static int quad(rt_tree* t, double qx, double qy, double qz, double ux, double uy, double uz,
                double vx, double vy, double vz, int mat) { /* NewQuad objects.go:129 */
  const double Q[3] = {qx, qy, qz}, u[3] = {ux, uy, uz}, v[3] = {vx, vy, vz};
  return must(rt_new_quad(t, Q, u, v, mat), "quad");
}
static int box(rt_tree* t, double x, double y, double z, int mat) { /* NewBox objects.go:208 */
  const double a[3] = {0, 0, 0}, b[3] = {x, y, z};
  return must(rt_new_box(t, a, b, mat), "box");
}
static int placed(rt_tree* t, int obj, double deg, double x, double y, double z) {
  const double off[3] = {x, y, z}; /* Translate(RotateY(obj, deg), off) transformation.go:20,48 */
  return must(rt_translate(t, must(rt_rotate_y(t, obj, deg), "rotate_y"), off), "translate");
}

/* cornellBox, main.go:278-320 (cornell_c99.c's) */
static void cornell(rt_tree* t, int* world_out, int* lights_out, rt_camera* c) {
  int world = must(rt_new_list(t), "list");
  int red = lambertian(t, .65, .05, .05), white = lambertian(t, .73, .73, .73);
  int green = lambertian(t, .12, .45, .15), lm = light(t, 15, 15, 15);
  int lights, b1, b2;
  must(rt_list_add(t, world, quad(t, 555, 0, 0, 0, 555, 0, 0, 0, 555, green)), "add");
  must(rt_list_add(t, world, quad(t, 0, 0, 0, 0, 555, 0, 0, 0, 555, red)), "add");
  must(rt_list_add(t, world, quad(t, 0, 0, 0, 555, 0, 0, 0, 0, 555, white)), "add");
  must(rt_list_add(t, world, quad(t, 555, 555, 555, -555, 0, 0, 0, 0, -555, white)), "add");
  must(rt_list_add(t, world, quad(t, 0, 0, 555, 555, 0, 0, 0, 555, 0, white)), "add");
  lights = must(rt_new_list(t), "list");
  must(rt_list_add(t, lights, quad(t, 343, 550, 332, -130, 0, 0, 0, 0, -105, lm)), "add");
  must(rt_list_add(t, world, lights), "add");
  b1 = placed(t, box(t, 165, 330, 165, white), 15, 265, 0, 295);
  b2 = placed(t, box(t, 165, 165, 165, white), -18, 130, 0, 65);
  must(rt_list_add(t, world, b1), "add");
  must(rt_list_add(t, world, b2), "add");
  memset(c, 0, sizeof *c);
  c->aspect_ratio = 1.0;
  c->width = 600;
  c->samples_per_pixel = 100;
  c->max_depth = 50;
  c->vertical_fov = 40;
  c->positioned = 1; /* PositionCamera(lookFrom, lookAt, vup) camera.go:65-81 */
  c->look_from[0] = 278, c->look_from[1] = 278, c->look_from[2] = -800;
  c->look_at[0] = 278, c->look_at[1] = 278, c->look_at[2] = 0;
  c->vup[1] = 1;
  *world_out = must(rt_build_bvh(t, world), "bvh"); /* BuildBVH bvh.go:21 */
  *lights_out = lights;
}

/* look_from turned about the vup axis through look_at by `degrees` (Rodrigues' formula), rtbench's
 * -orbit operation for operation */
static rt_camera orbit(const rt_camera* cam0, double degrees) {
  rt_camera cam = *cam0;
  const double pi = 3.14159265358979323846;
  const double th = degrees * pi / 180.0, co = cos(th), si = sin(th);
  const double* up = cam0->vup;
  const double ul = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
  double k[3], v[3], kxv[3], kv;
  int i;
  for (i = 0; i < 3; ++i) k[i] = up[i] / ul, v[i] = cam0->look_from[i] - cam0->look_at[i];
  kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
  kxv[0] = k[1] * v[2] - k[2] * v[1], kxv[1] = k[2] * v[0] - k[0] * v[2], kxv[2] = k[0] * v[1] - k[1] * v[0];
  for (i = 0; i < 3; ++i) cam.look_from[i] = cam0->look_at[i] + (v[i] * co + kxv[i] * si + k[i] * kv * (1.0 - co));
  return cam;
}

int main(int argc, char** argv) {
  rt_tree* tree = NULL;
  rt_scene* scene = NULL;
  rt_pipeline* pipe = NULL;
  rt_pipeline_opts po;
  rt_render_opts opts;
  rt_camera cam0;
  uint64_t seed;
  double degrees;
  int world, lights, k, i;
  if (argc != 5) {
    fprintf(stderr, "usage: %s W SEED DEGREES PREFIX\n", argv[0]);
    return 2;
  }
  must(rt_tree_create(&tree), "tree");
  cornell(tree, &world, &lights, &cam0);
  must(rt_scene_create(tree, world, lights, &scene), "scene");
  cam0.width = atoi(argv[1]);
  cam0.samples_per_pixel = 4;
  seed = strtoull(argv[2], NULL, 10);
  degrees = atof(argv[3]);

  /* the history and the filter, owned on the device by one object: directly seen lights kept out
   * of the history (EMIT), the variance from the luminance moments (the frames have one pass), the
   * split variance-guided filter demodulating by the surface albedo; everything else the defaults */
  memset(&po, 0, sizeof po);
  po.temporal = 1;
  po.mode = RT_REPROJECT_EMIT;
  po.moments = 1;
  po.filter = RT_PIPE_FILTER_VAR;
  po.split_emitters = 1;
  po.vopts.demodulate = 1;
  must(rt_pipeline_create(&po, &pipe), "pipeline"); /* touches no device */
  memset(&opts, 0, sizeof opts);
  opts.nranks = SHARES;

  for (k = 0; k < FRAMES; ++k) {
    const rt_camera cam = orbit(&cam0, degrees * (double)k);
    rt_accum* accs[SHARES];
    rt_stats stats;
    rt_pipeline_info info;
    char name[1024];
    char* text;
    int64_t len;
    FILE* f;
    for (i = 0; i < SHARES; ++i) { /* rows i, i + SHARES, ... of the frame, on DEVICES[i] */
      opts.rank = i;
      opts.device = DEVICES[i];
      must(rt_accum_create(scene, &cam, &opts, 1, &accs[i]), "accum");
      must(rt_accum_set_features(accs[i], RT_ACCUM_FEAT_GUIDES | RT_ACCUM_FEAT_EMIT), "features");
    }
    must(rt_accum_add_shares(accs, SHARES, seed + (uint64_t)k, &stats), "pass"); /* a host thread per share */
    must(rt_pipeline_push_shares(pipe, accs, SHARES), "push"); /* resolve, gather, reproject, filter: on the devices */
    for (i = 0; i < SHARES; ++i) must(rt_accum_destroy(accs[i]), "accum destroy"); /* the pipeline keeps nothing of them */
    len = rt_pipeline_ppm(pipe, NULL, 0); /* the size, then the text: one copy */
    must((int)(len < 0 ? len : 0), "ppm size");
    text = (char*)malloc((size_t)len);
    if (!text || rt_pipeline_ppm(pipe, text, len) != len) return 2;
    snprintf(name, sizeof name, "%s_%03d.ppm", argv[4], k);
    f = fopen(name, "wb");
    if (!f || fwrite(text, 1, (size_t)len, f) != (size_t)len || fclose(f) != 0) return 2;
    free(text);
    must(rt_pipeline_info_get(pipe, &info), "info");
    printf("{\"frame\": %d, \"shares\": %d, \"rows\": %d, \"width\": %d, \"height\": %d, \"had_history\": %d, \"device_bytes\": %llu, "
           "\"allocations\": %llu, \"ppm_bytes\": %lld}\n",
           k, SHARES, (int)stats.rows, (int)info.width, (int)info.height, (int)info.had_history, (unsigned long long)info.device_bytes,
           (unsigned long long)info.allocations, (long long)len);
  }
  must(rt_scene_destroy(scene), "destroy"); /* the scene may go first */
  must(rt_pipeline_destroy(pipe), "pipeline destroy");
  must(rt_tree_destroy(tree), "destroy");
  return 0;
}
