// rtbench: the reference's command line (main.go:414-478) over the C ABI.
//
//   rtbench [-o image.ppm] [-N cores] [-S scene] [-cpuprofile file] [extensions]
//
// Same flags, defaults and effects as main.go: -S picks the scene function
// (1 book1 .. 8 model, main.go:447-472; anything else is defaultScene, which
// renders nothing, so the output file is created and left empty), -o names the
// output file (created before the render, main.go:434-439), -N is
// Camera.MaxThreads (the GPU path ignores it; kept in rt_camera.max_threads).
// Flag syntax follows Go's flag package: -name value, -name=value, --name;
// bool flags take no value; parsing stops at "--" or the first non-flag;
// an unknown flag or a bad value prints the usage and exits 2, -h exits 0.
//
// Extensions beyond main.go (defaults leave the reference scene unchanged):
// -device, -width, -spp, -depth (camera overrides), -seed (render seed),
// -tree-seed (the scene's rand seed), -mode auto|fused|wavefront, -assets DIR,
// -progress (a progress line on stderr, the reference's bubbletea bar,
// camera.go:106-108), -slices N (rt_progress granularity), -stats (one JSON
// line of rt_stats on stderr), -denoise (feature pass at min(spp, 16) samples, then
// the a-trous denoiser before the PPM is written; prints the statistics line with
// both times), -denoise-var (the same with the variance-guided filter, rt_denoise_var, fed from
// the pass accumulator's variance: needs -passes N >= 2 or -until; the statistics line gains
// "denoise_var": 1), -split-emitters (with either: rt_render_aov_emit and the _emit filter, so
// directly seen lights stay out of the filter; alone a usage error; -aov then also writes
// PREFIX_emission.ppm and PREFIX_coverage.ppm; the statistics line gains "split_emitters": 1),
// -aov PREFIX (writes PREFIX_albedo.ppm, PREFIX_normal.ppm as
// n * 0.5 + 0.5 and PREFIX_depth.ppm normalised to the image maximum, through the
// same PPM writer), -passes N (the image as the exact mean of N passes of -spp samples each,
// seeds seed .. seed + N - 1, through the pass accumulator; -passes 1 writes the plain
// render's bytes), -until E (stop once the accumulator's rel_error is <= E, checked from the
// second pass on; at most -passes passes, 1024 without it).  With either, -progress reports
// passes and the statistics line gains passes, rel_error and ms_accum.  -adaptive E (adaptive
// passes: every pass is rt_accum_select + rt_accum_add_active, so whole passes while some pixel
// has fewer than the library's min_passes, then passes over the tiles whose error figure is
// above E only, until none is left or -passes, default 1024, is reached; composes with
// -denoise[-var], -aov and -o; the statistics line gains active_last, samples_total and
// samples_full), -accum-features (with -passes / -until / -adaptive: the accumulator keeps the
// feature sums of its passes' own camera samples, rt_accum_set_features, and the denoisers and
// -aov take those guides instead of a separate feature pass; without an accumulating flag a
// usage error; the statistics line gains "accum_features": 1), -frames N -orbit DEG (N frames, frame k
// with the camera's look_from turned about the vup axis through look_at by k * DEG degrees and written
// to the -o name with _%03d before the extension, -aov's prefix with the same suffix; one statistics
// line per frame, with "frame": k; without -temporal the frames are independent), -temporal (with
// -accum-features and an accumulating flag, else a usage error: each frame's accumulator mean, variance
// and guides go through rt_reproject against the history of the frames before it, every pixel of a frame
// weighing its passes, before -denoise-var and the writer, and the result is the next frame's history;
// the host entry, which stages through the device and gives rt_reproject_device's bits: this client
// links no HIP runtime to own device buffers with; the statistics line gains "temporal": 1 and
// ms_reproject), -temporal-emit (as -temporal, and needs -split-emitters too, else a usage error: the
// stage runs through rt_reproject_emit with the accumulator's emission and coverage, which are kept
// with the history; the statistics line also gains "temporal_emit": 1), -aov-media (with -aov, -denoise[-var] or
// -accum-features, else a usage error: the feature buffers are of the samples' first EVENTS, constant
// media traced as the render's camera vertex traces them, through rt_render_aov_media or an accumulator
// with RT_ACCUM_FEAT_MEDIA; -aov also writes PREFIX_scatter.ppm, the scatter fraction as grey; the
// statistics line gains "aov_media": 1; without the flag every byte written is what it was),
// -counts FILE (with -adaptive: the passes per pixel as grey, count / max).  -cpuprofile has no pprof to drive on the GPU path: the file
// receives the same JSON statistics instead.
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rt_abi.h"

namespace {

struct Flag {
  const char* name;
  const char* usage;
  enum Kind { STR, INT, U64, BOOL, F64 } kind;
  void* dst;
  const char* def;  // shown in the usage, Go style
};

struct Args {
  std::string cpuprofile, out = "image.ppm", mode = "auto", assets, aov, counts;
  long long N = 1, S = -1, device = 0, width = 0, spp = 0, depth = 0, slices = 0, passes = 0;
  double until = 0.0, adaptive = 0.0;
  bool adaptive_set = false;
  unsigned long long seed = 1, tree_seed = 1;
  bool progress = false, stats = false, denoise = false, denoise_var = false, split_emitters = false;
  bool accum_features = false, temporal = false, temporal_emit = false, aov_media = false;
  long long frames = 0;
  double orbit = 0.0;
};

std::vector<Flag> flags(Args& a) {
  return {
      {"N", "Set the number of cores to allocate to rendering", Flag::INT, &a.N, "1"},
      {"S", "Set the scene to render, default will render a custom scene function", Flag::INT,
       &a.S, "-1"},
      {"accum-features", "with -passes, -until or -adaptive: the denoiser's and -aov's feature buffers come from the accumulator (the passes' own camera samples), not from a separate feature pass",
       Flag::BOOL, &a.accum_features, ""},
      {"adaptive", "adaptive passes: after the first whole passes, resample only the tiles whose relative error is > E (at most -passes, default 1024)",
       Flag::F64, &a.adaptive, ""},
      {"aov-media", "with -aov, -denoise[-var] or -accum-features: trace constant media in the feature buffers (first-event guides); -aov also writes PREFIX_scatter.ppm",
       Flag::BOOL, &a.aov_media, ""},
      {"aov", "write PREFIX_albedo.ppm, PREFIX_normal.ppm and PREFIX_depth.ppm (first-hit feature buffers)",
       Flag::STR, &a.aov, ""},
      {"assets", "directory holding earthmap.jpg / dragon.obj (default: <exe dir>/../assets)",
       Flag::STR, &a.assets, ""},
      {"counts", "with -adaptive: write the passes per pixel as a grey image (count / largest count)", Flag::STR,
       &a.counts, ""},
      {"cpuprofile", "Write cpu profile to file (here: render statistics as JSON)", Flag::STR,
       &a.cpuprofile, ""},
      {"denoise", "denoise the image (a-trous filter guided by the feature buffers) before it is written",
       Flag::BOOL, &a.denoise, ""},
      {"denoise-var", "denoise with the variance-guided filter fed from the accumulator's variance (needs -passes N >= 2 or -until)",
       Flag::BOOL, &a.denoise_var, ""},
      {"depth", "override Camera.MaxDepth (0 = the scene's)", Flag::INT, &a.depth, "0"},
      {"device", "HIP device ordinal", Flag::INT, &a.device, "0"},
      {"frames", "render N frames, frame k to the -o name with _00k before the extension (see -orbit)", Flag::INT,
       &a.frames, "0"},
      {"mode", "kernel strategy: auto, fused or wavefront", Flag::STR, &a.mode, "auto"},
      {"o", "Specify a custom output file", Flag::STR, &a.out, "image.ppm"},
      {"orbit", "with -frames: turn the camera's look_from about the vup axis through look_at by DEG degrees per frame",
       Flag::F64, &a.orbit, "0"},
      {"passes", "render N passes of -spp samples each (seeds seed .. seed+N-1) and write their exact mean",
       Flag::INT, &a.passes, "0"},
      {"progress", "print render progress on stderr", Flag::BOOL, &a.progress, ""},
      {"seed", "render seed (Philox key)", Flag::U64, &a.seed, "1"},
      {"slices", "progress granularity: launches per render (0 = 20 with -progress)", Flag::INT,
       &a.slices, "0"},
      {"split-emitters", "with -denoise or -denoise-var: keep directly seen lights out of the filter (emission split); -aov also writes PREFIX_emission.ppm and PREFIX_coverage.ppm",
       Flag::BOOL, &a.split_emitters, ""},
      {"spp", "override Camera.SamplesPerPixel (0 = the scene's)", Flag::INT, &a.spp, "0"},
      {"stats", "print render statistics (JSON) on stderr", Flag::BOOL, &a.stats, ""},
      {"temporal", "with -accum-features and -passes / -until / -adaptive: blend each frame with the reprojected history of the frames before it (rt_reproject)",
       Flag::BOOL, &a.temporal, ""},
      {"temporal-emit", "as -temporal, with directly seen lights kept out of the history (rt_reproject_emit); needs -split-emitters too",
       Flag::BOOL, &a.temporal_emit, ""},
      {"tree-seed", "seed of the scene builder's rand (main.go's math/rand)", Flag::U64,
       &a.tree_seed, "1"},
      {"until", "add passes until the image's relative standard error is <= E (at most -passes, default 1024)",
       Flag::F64, &a.until, "0"},
      {"width", "override Camera.Width (0 = the scene's)", Flag::INT, &a.width, "0"},
  };
}

void usage(const char* prog, const std::vector<Flag>& fl) {
  fprintf(stderr, "Usage of %s:\n", prog);
  for (const Flag& f : fl) {
    const char* ty = f.kind == Flag::STR ? " string" : f.kind == Flag::INT ? " int"
                     : f.kind == Flag::U64 ? " uint" : f.kind == Flag::F64 ? " float" : "";
    fprintf(stderr, "  -%s%s\n    \t%s", f.name, ty, f.usage);
    if (f.def && *f.def && !((f.kind == Flag::INT || f.kind == Flag::F64) && !strcmp(f.def, "0")))
      fprintf(stderr, f.kind == Flag::STR ? " (default \"%s\")" : " (default %s)", f.def);
    fprintf(stderr, "\n");
  }
}

// strconv.ParseInt(s, 0, 64) / ParseUint / ParseBool as flag.Value.Set uses them
bool set_value(const Flag& f, const std::string& v) {
  errno = 0;
  char* end = nullptr;
  switch (f.kind) {
    case Flag::STR: *(std::string*)f.dst = v; return true;
    case Flag::INT: {
      long long x = strtoll(v.c_str(), &end, 0);
      if (v.empty() || *end || errno) return false;
      *(long long*)f.dst = x;
      return true;
    }
    case Flag::U64: {
      if (v.empty() || v[0] == '-') return false;
      unsigned long long x = strtoull(v.c_str(), &end, 0);
      if (*end || errno) return false;
      *(unsigned long long*)f.dst = x;
      return true;
    }
    case Flag::F64: {
      double x = strtod(v.c_str(), &end);
      if (v.empty() || *end || errno) return false;
      *(double*)f.dst = x;
      return true;
    }
    case Flag::BOOL: {
      static const char* t[] = {"1", "t", "T", "true", "TRUE", "True"};
      static const char* n[] = {"0", "f", "F", "false", "FALSE", "False"};
      for (const char* s : t) if (v == s) return *(bool*)f.dst = true, true;
      for (const char* s : n) if (v == s) return *(bool*)f.dst = false, true;
      return false;
    }
  }
  return false;
}

// flag.FlagSet.Parse with ExitOnError: returns the exit code, or -1 to go on
int parse(int argc, char** argv, Args& a) {
  std::vector<Flag> fl = flags(a);
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    if (s.size() < 2 || s[0] != '-') break;  // first non-flag argument
    size_t dashes = s[1] == '-' ? 2 : 1;
    if (dashes == 2 && s.size() == 2) break;  // "--" terminates
    std::string name = s.substr(dashes), val;
    bool has_val = false;
    if (name.empty() || name[0] == '-' || name[0] == '=') {
      fprintf(stderr, "bad flag syntax: %s\n", s.c_str());
      usage(argv[0], fl);
      return 2;
    }
    size_t eq = name.find('=');
    if (eq != std::string::npos) val = name.substr(eq + 1), name = name.substr(0, eq), has_val = true;
    if (name == "h" || name == "help") {
      usage(argv[0], fl);
      return 0;
    }
    const Flag* f = nullptr;
    for (const Flag& c : fl)
      if (name == c.name) f = &c;
    if (!f) {
      fprintf(stderr, "flag provided but not defined: -%s\n", name.c_str());
      usage(argv[0], fl);
      return 2;
    }
    if (f->kind == Flag::BOOL && !has_val) {
      val = "true";
    } else if (!has_val) {
      if (i + 1 >= argc) {
        fprintf(stderr, "flag needs an argument: -%s\n", name.c_str());
        usage(argv[0], fl);
        return 2;
      }
      val = argv[++i];
    }
    if (!set_value(*f, val)) {
      fprintf(stderr, "invalid value \"%s\" for flag -%s: parse error\n", val.c_str(),
              name.c_str());
      usage(argv[0], fl);
      return 2;
    }
    if (name == "adaptive") a.adaptive_set = true;
  }
  if (a.adaptive_set && !(a.adaptive > 0.0)) {
    fprintf(stderr, "invalid value for flag -adaptive: the error threshold must be > 0\n");
    usage(argv[0], fl);
    return 2;
  }
  if (!a.counts.empty() && !a.adaptive_set) {
    fprintf(stderr, "-counts needs -adaptive\n");
    usage(argv[0], fl);
    return 2;
  }
  return -1;
}

std::string exe_dir() {
  char buf[4096];
  ssize_t n = readlink("/proc/self/exe", buf, sizeof buf - 1);
  if (n <= 0) return ".";
  buf[n] = 0;
  std::string p = buf;
  size_t k = p.rfind('/');
  return k == std::string::npos ? "." : p.substr(0, k);
}

int fail(const char* what, int rc) {
  fprintf(stderr, "rtbench: %s failed (%d): %s\n", what, rc, rt_last_error());
  return 1;
}

std::string stats_json(const rt_stats& st, const rt_camera_derived& d, const char* scene,
                       double wall_s, int aov_samples, double ms_aov, double ms_denoise,
                       const rt_accum_info* acc, double ms_accum, bool denoise_var,
                       const rt_adapt_info* ad = nullptr, bool split_emitters = false,
                       bool accum_features = false, int frame = -1, bool temporal = false,
                       double ms_reproject = 0.0, bool temporal_emit = false, bool aov_media = false) {
  char b[1280], extra[200] = "", extra2[200] = "", extra4[160] = "";
  if (frame >= 0) snprintf(extra4, sizeof extra4, "\"frame\": %d, ", frame);
  if (temporal) snprintf(extra4 + strlen(extra4), sizeof extra4 - strlen(extra4), "\"temporal\": 1, \"ms_reproject\": %.3f, ", ms_reproject);
  if (temporal_emit) snprintf(extra4 + strlen(extra4), sizeof extra4 - strlen(extra4), "\"temporal_emit\": 1, ");
  if (aov_media) snprintf(extra4 + strlen(extra4), sizeof extra4 - strlen(extra4), "\"aov_media\": 1, ");
  const std::string extra3s = std::string(split_emitters ? "\"split_emitters\": 1, " : "") +
                              (accum_features ? "\"accum_features\": 1, " : "") + extra4;
  const char* extra3 = extra3s.c_str();
  if (acc)  // -passes / -until
    snprintf(extra, sizeof extra, "\"passes\": %d, \"rel_error\": %.6g, \"ms_accum\": %.3f, %s", acc->passes,
             acc->rel_error, ms_accum, denoise_var ? "\"denoise_var\": 1, " : "");
  if (acc && ad)  // -adaptive
    snprintf(extra2, sizeof extra2, "\"active_last\": %" PRIu64 ", \"samples_total\": %" PRIu64
             ", \"samples_full\": %" PRIu64 ", ", ad->active_pixels, ad->total_samples,
             (uint64_t)acc->passes * (uint64_t)(d.spp_sqrt * d.spp_sqrt) * (uint64_t)d.width * (uint64_t)d.height);
  snprintf(b, sizeof b,
           "{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %d, \"max_depth\": %d, "
           "\"samples\": %" PRIu64 ", \"segments\": %" PRIu64 ", \"ms_render\": %.3f, "
           "\"samples_per_s\": %.6g, \"mode\": %d, \"tree_width\": %d, \"chunk_samples\": %d, "
           "\"aov_samples\": %d, \"ms_aov\": %.3f, \"ms_denoise\": %.3f, %s%s%s\"wall_s\": %.3f}",
           scene, d.width, d.height, d.spp_sqrt * d.spp_sqrt, d.max_depth, st.samples,
           st.segments, st.ms_total, st.ms_total > 0 ? st.samples / (st.ms_total * 1e-3) : 0.0,
           st.mode, st.tree_width, st.chunk_samples, aov_samples, ms_aov, ms_denoise, extra, extra2, extra3, wall_s);
  return b;
}

// one image through the PPM writer (camera.go:160 + PrintColor) into `path`
int write_ppm(const std::vector<float>& img, int w, int h, FILE* f, const char* path) {
  int64_t n = rt_format_ppm(img.data(), w, h, nullptr, 0);
  std::vector<char> text((size_t)(n > 0 ? n : 0));
  if (n < 0 || rt_format_ppm(img.data(), w, h, text.data(), n) != n) return fail("rt_format_ppm", (int)n);
  if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) {
    fprintf(stderr, "rtbench: writing %s failed\n", path);
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  int rc = parse(argc, argv, a);
  if (rc >= 0) return rc;
  auto t0 = std::chrono::steady_clock::now();
  // the variance comes from the passes: one pass has none (checked before the file is created)
  if (a.denoise_var && !(a.passes >= 2 || ((a.until > 0.0 || a.adaptive_set) && a.passes == 0))) {
    fprintf(stderr, "-denoise-var needs -passes N with N >= 2, or -until / -adaptive\n");
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.split_emitters && !a.denoise && !a.denoise_var) {  // nothing to split for
    fprintf(stderr, "-split-emitters needs -denoise or -denoise-var\n");
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.accum_features && !(a.passes > 0 || a.until > 0.0 || a.adaptive_set)) {  // no accumulator to keep them
    fprintf(stderr, "-accum-features needs -passes, -until or -adaptive\n");
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.temporal && !(a.accum_features && (a.passes > 0 || a.until > 0.0 || a.adaptive_set))) {  // no guides, no history
    fprintf(stderr, "-temporal needs -accum-features and -passes, -until or -adaptive\n");
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.temporal_emit && !(a.split_emitters && a.accum_features && (a.passes > 0 || a.until > 0.0 || a.adaptive_set))) {
    fprintf(stderr, "-temporal-emit needs -split-emitters, -accum-features and -passes, -until or -adaptive\n");  // no emit planes
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.aov_media && !(a.denoise || a.denoise_var || !a.aov.empty() || a.accum_features)) {  // no feature buffers
    fprintf(stderr, "-aov-media needs -aov, -denoise, -denoise-var or -accum-features\n");
    usage(argv[0], flags(a));
    return 2;
  }
  if (a.temporal_emit) a.temporal = true;  // the same stage, through rt_reproject_emit
  if (a.frames < 0 || a.frames > 999 || !(a.orbit == a.orbit)) {
    fprintf(stderr, "invalid value for flag -frames (0..999) / -orbit\n");
    usage(argv[0], flags(a));
    return 2;
  }
  const bool numbered = a.frames > 0;  // -frames: frame k goes to the -o name with _00k before the extension
  const int n_frames = numbered ? (int)a.frames : 1;
  auto frame_name = [&](const std::string& name, int k, bool before_ext) {
    char tag[8];
    snprintf(tag, sizeof tag, "_%03d", k);
    const size_t slash = name.rfind('/'), dot = name.rfind('.');
    const bool ext = before_ext && dot != std::string::npos && (slash == std::string::npos || dot > slash);
    return ext ? name.substr(0, dot) + tag + name.substr(dot) : name + tag;
  };

  // main.go:434-439: the output file exists before anything renders
  const std::string out_first = numbered ? frame_name(a.out, 0, true) : a.out;
  FILE* out = fopen(out_first.c_str(), "wb");
  if (!out) {
    fprintf(stderr, "Error creating output file\n");
    return 1;
  }
  const char* scene = nullptr;
  if (a.S < 1 || a.S > 8 || rt_demo_scene_name((int)a.S, &scene) != RT_OK || !scene) {
    fclose(out);  // defaultScene (main.go:412-414): nothing rendered, empty file
    return 0;
  }
  int mode = a.mode == "auto" ? RT_MODE_AUTO : a.mode == "fused" ? RT_MODE_FUSED
             : a.mode == "wavefront" ? RT_MODE_WAVEFRONT : -1;
  if (mode < 0) {
    fprintf(stderr, "invalid value \"%s\" for flag -mode\n", a.mode.c_str());
    fclose(out);
    return 2;
  }
  std::string assets = a.assets.empty() ? exe_dir() + "/../assets" : a.assets;
  if (a.assets.empty() && getenv("RT_ASSET_DIR")) assets = getenv("RT_ASSET_DIR");

  rt_tree* tree = nullptr;
  rt_scene* sc = nullptr;
  if ((rc = rt_tree_create(&tree)) != RT_OK) return fail("rt_tree_create", rc);
  rt_tree_seed(tree, a.tree_seed);
  rt_camera cam;
  memset(&cam, 0, sizeof cam);
  int world = -1, lights = -1;
  if ((rc = rt_demo_scene(tree, scene, assets.c_str(), &cam, &world, &lights)) != RT_OK)
    return fail("rt_demo_scene", rc);
  cam.max_threads = (int32_t)a.N;
  if (a.width > 0) cam.width = (int32_t)a.width;
  if (a.spp > 0) cam.samples_per_pixel = (int32_t)a.spp;
  if (a.depth > 0) cam.max_depth = (int32_t)a.depth;
  rt_camera_derived d;
  if ((rc = rt_camera_derive(&cam, &d)) != RT_OK) return fail("rt_camera_derive", rc);
  if ((rc = rt_scene_create(tree, world, lights, &sc)) != RT_OK)
    return fail("rt_scene_create", rc);

  // -temporal: the history (the frames before this one, reprojected and blended) and its camera
  const size_t n_px = (size_t)d.width * d.height;
  std::vector<float> h_rgb, h_var, h_count, h_normal, h_depth, h_emission, h_coverage, count;
  rt_camera h_cam;
  bool have_history = false;
  const rt_camera cam0 = cam;
  const std::string aov0 = a.aov;

  for (int frame = 0; frame < n_frames; ++frame) {
  double ms_reproject = 0.0;
  std::string out_name = a.out;
  if (numbered) {
    out_name = frame_name(a.out, frame, true);
    if (!aov0.empty()) a.aov = frame_name(aov0, frame, false);
    if (frame > 0 && !(out = fopen(out_name.c_str(), "wb"))) {
      fprintf(stderr, "Error creating output file\n");
      return 1;
    }
    // -orbit: look_from turned about the vup axis through look_at (Rodrigues' formula)
    double from[3] = {0, 0, 0}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0};
    if (cam0.positioned)
      for (int i = 0; i < 3; ++i) from[i] = cam0.look_from[i], at[i] = cam0.look_at[i], up[i] = cam0.vup[i];
    const double th = a.orbit * (double)frame * M_PI / 180.0, co = cos(th), si = sin(th);
    const double ul = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
    const double k[3] = {up[0] / ul, up[1] / ul, up[2] / ul};
    const double v[3] = {from[0] - at[0], from[1] - at[1], from[2] - at[2]};
    const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
    const double kxv[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
    for (int i = 0; i < 3; ++i) {
      cam.look_from[i] = at[i] + (v[i] * co + kxv[i] * si + k[i] * kv * (1.0 - co));
      cam.look_at[i] = at[i];
      cam.vup[i] = up[i];
    }
    cam.positioned = 1;
  }

  rt_render_opts o;
  memset(&o, 0, sizeof o);
  o.seed = a.seed;
  o.device = (int32_t)a.device;
  o.nranks = 1;
  o.mode = mode;
  o.trace_pixel = -1;
  o.progress_slices = (int32_t)(a.slices > 0 ? a.slices : a.progress ? 20 : 0);
  std::vector<float> rgb((size_t)d.width * d.height * 3), var(a.denoise_var || a.temporal ? (size_t)d.width * d.height : 0);
  rt_stats st;
  memset(&st, 0, sizeof st);

  // -passes / -until: the image is the accumulator's mean over the passes
  const bool accumulate = a.passes > 0 || a.until > 0.0 || a.adaptive_set;
  if (a.passes < 0 || a.passes > 0x7FFFFFFF || !(a.until >= 0.0)) {
    fprintf(stderr, "invalid value for flag -passes / -until\n");
    fclose(out);
    return 2;
  }
  const int32_t pass_cap = (int32_t)(a.passes > 0 ? a.passes : 1024);
  rt_accum* acc = nullptr;
  rt_accum_info ai;
  memset(&ai, 0, sizeof ai);
  rt_adapt_info adi;
  memset(&adi, 0, sizeof adi);
  rt_adapt_opts ado;
  memset(&ado, 0, sizeof ado);  // the library defaults: tile 8, min_passes 4, lum_floor 1e-2
  ado.rel_error = a.adaptive;
  double ms_accum = 0.0;
  if (accumulate && (rc = rt_accum_create(sc, &cam, &o, pass_cap, &acc)) != RT_OK)
    return fail("rt_accum_create", rc);
  if (a.accum_features &&
      (rc = rt_accum_set_features(acc, RT_ACCUM_FEAT_GUIDES | (a.split_emitters ? RT_ACCUM_FEAT_EMIT : 0u) |
                                          (a.aov_media ? RT_ACCUM_FEAT_MEDIA : 0u))) != RT_OK)
    return fail("rt_accum_set_features", rc);

  bool counts_failed = false;
  std::atomic<bool> rendering{true};
  std::atomic<int> pass_no{0};
  std::thread bar;
  if (a.progress) {
    bar = std::thread([&] {
      uint64_t done = 0, total = 0;
      while (rendering.load()) {
        if (rt_progress(sc, &done, &total) == RT_OK && total) {
          if (accumulate)
            fprintf(stderr, "\rrendering %s: pass %d of %d, %5.1f%%", scene, pass_no.load() + 1, pass_cap,
                    100.0 * done / total);
          else
            fprintf(stderr, "\rrendering %s: %5.1f%%", scene, 100.0 * done / total);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
      }
    });
  }
  const char* what = "rt_render";
  if (!accumulate) {
    rc = rt_render(sc, &cam, &o, rgb.data(), &st);
  } else {
    auto tp = std::chrono::steady_clock::now();
    for (int32_t p = 0; p < pass_cap && rc == RT_OK; ++p) {
      rt_stats sp;
      pass_no = p;
      if (a.adaptive_set) {  // the noisy tiles only (Accumulator.render_adaptive); every tile at first
        uint64_t n_active = 0;
        what = "rt_accum_select";
        if ((rc = rt_accum_select(acc, &ado, &n_active)) != RT_OK || n_active == 0) break;
        what = "rt_accum_add_active";
        if ((rc = rt_accum_add_active(acc, a.seed + (uint64_t)p, &sp)) != RT_OK) break;
      } else {
        what = "rt_accum_add";
        if ((rc = rt_accum_add(acc, a.seed + (uint64_t)p, &sp)) != RT_OK) break;
      }
      const uint64_t samples = st.samples + sp.samples, segments = st.segments + sp.segments;
      const double ms = st.ms_total + sp.ms_total;
      st = sp;  // the last pass's, with the totals over the passes
      st.samples = samples;
      st.segments = segments;
      st.ms_total = ms;
      if (a.until > 0.0 && p >= 1) {
        what = "rt_accum_info_get";
        if ((rc = rt_accum_info_get(acc, &ai)) != RT_OK || ai.rel_error <= a.until) break;
      }
    }
    if (rc == RT_OK) {
      what = "rt_accum_resolve";
      if ((rc = rt_accum_resolve(acc, rgb.data(), a.denoise_var || a.temporal ? var.data() : nullptr)) == RT_OK) rc = rt_accum_info_get(acc, &ai);
    }
    if (rc == RT_OK && a.adaptive_set) {
      what = "rt_accum_adapt_info";
      rc = rt_accum_adapt_info(acc, &adi);
      if (rc == RT_OK && !a.counts.empty()) {
        const size_t np = (size_t)d.width * d.height;
        std::vector<int32_t> cnt(np);
        what = "rt_accum_counts";
        if ((rc = rt_accum_counts(acc, cnt.data())) == RT_OK) {
          std::vector<float> cimg(3 * np);
          for (size_t i = 0; i < np; ++i)
            cimg[3 * i] = cimg[3 * i + 1] = cimg[3 * i + 2] = adi.max_count > 0 ? (float)cnt[i] / (float)adi.max_count : 0.0f;
          counts_failed = write_ppm(cimg, d.width, d.height, fopen(a.counts.c_str(), "wb"), a.counts.c_str()) != 0;
        }
      }
    }
    ms_accum = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
  }
  rendering = false;
  if (bar.joinable()) bar.join();
  if (a.progress && accumulate)
    fprintf(stderr, "\rrendering %s: %d passes, 100.0%%      \n", scene, ai.passes);
  else if (a.progress)
    fprintf(stderr, "\rrendering %s: 100.0%%\n", scene);
  if (rc != RT_OK) return fail(what, rc);
  if (counts_failed) {  // (reported by write_ppm; after the progress thread has been joined)
    rt_scene_destroy(sc);
    rt_tree_destroy(tree);
    return 1;
  }

  // -denoise / -aov: the feature buffers of the same camera rays, then the filter
  int aov_samples = 0;
  double ms_aov = 0.0, ms_denoise = 0.0;
  if (a.denoise || a.denoise_var || !a.aov.empty() || a.temporal) {
    const size_t np = (size_t)d.width * d.height;
    std::vector<float> albedo(3 * np), normal(3 * np), depth(np);
    rt_aov f = {albedo.data(), normal.data(), depth.data(), nullptr};
    aov_samples = d.spp_sqrt * d.spp_sqrt < 16 ? d.spp_sqrt * d.spp_sqrt : 16;
    if (a.accum_features) aov_samples = d.spp_sqrt * d.spp_sqrt;  // of every pass the pixel took
    rt_stats sa;
    auto ta = std::chrono::steady_clock::now();
    // -split-emitters: the split feature pass and the split filter
    std::vector<float> emission(a.split_emitters ? 3 * np : 0), salbedo(a.split_emitters ? 3 * np : 0),
        coverage(a.split_emitters ? np : 0);
    rt_aov_emit fe = {emission.data(), salbedo.data(), coverage.data()};
    // -aov-media: the first-event buffers and the scatter plane
    std::vector<float> scatter(a.aov_media ? np : 0);
    const rt_aov_media fm = {scatter.data()};
    if (a.aov_media && a.accum_features) {
      if ((rc = rt_accum_resolve_aov_media(acc, &f, a.split_emitters ? &fe : nullptr, &fm)) != RT_OK)
        return fail("rt_accum_resolve_aov_media", rc);
    } else if (a.aov_media) {
      if ((rc = rt_render_aov_media(sc, &cam, &o, aov_samples, &f, a.split_emitters ? &fe : nullptr, &fm, &sa)) != RT_OK)
        return fail("rt_render_aov_media", rc);
    } else if (a.accum_features) {  // the guides of the passes' own samples: no feature pass
      if ((rc = rt_accum_resolve_aov(acc, &f, a.split_emitters ? &fe : nullptr)) != RT_OK)
        return fail("rt_accum_resolve_aov", rc);
    } else if (a.split_emitters) {
      if ((rc = rt_render_aov_emit(sc, &cam, &o, aov_samples, &f, &fe, &sa)) != RT_OK)
        return fail("rt_render_aov_emit", rc);
    } else if ((rc = rt_render_aov(sc, &cam, &o, aov_samples, &f, &sa)) != RT_OK) {
      return fail("rt_render_aov", rc);
    }
    ms_aov = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
    if (a.temporal) {  // the history into this frame's camera, then this frame as the new history
      auto tr = std::chrono::steady_clock::now();
      count.assign(n_px, (float)ai.passes);
      if (have_history) {
        const rt_frame prev = {h_rgb.data(), h_var.data(), h_count.data(), h_normal.data(), h_depth.data(), 0.0f, 0};
        const rt_frame cur = {rgb.data(), var.data(), nullptr, normal.data(), depth.data(), (float)ai.passes, 0};
        const rt_frame res = {rgb.data(), var.data(), count.data(), nullptr, nullptr, 0.0f, 0};
        const rt_aov_emit prev_emit = {h_emission.data(), nullptr, h_coverage.data()};
        const rt_aov_emit cur_emit = {emission.data(), nullptr, coverage.data()};
        if (a.temporal_emit) {
          if ((rc = rt_reproject_emit(&h_cam, &prev, &prev_emit, &cam, &cur, &cur_emit, d.width, d.height, nullptr,
                                      &res)) != RT_OK)
            return fail("rt_reproject_emit", rc);
        } else if ((rc = rt_reproject(&h_cam, &prev, &cam, &cur, d.width, d.height, nullptr, &res)) != RT_OK) {
          return fail("rt_reproject", rc);
        }
      }
      h_rgb = rgb, h_var = var, h_count = count, h_normal = normal, h_depth = depth;
      if (a.temporal_emit) h_emission = emission, h_coverage = coverage;
      h_cam = cam;
      have_history = true;
      ms_reproject = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();
    }
    if (a.denoise_var) {
      rt_denoise_var_opts vopt;
      memset(&vopt, 0, sizeof vopt);  // the library defaults
      vopt.demodulate = 1;
      auto td = std::chrono::steady_clock::now();
      if (a.split_emitters) {
        if ((rc = rt_denoise_var_emit(rgb.data(), var.data(), &f, &fe, d.width, d.height, &vopt, rgb.data(),
                                      nullptr)) != RT_OK)
          return fail("rt_denoise_var_emit", rc);
      } else if ((rc = rt_denoise_var(rgb.data(), var.data(), &f, d.width, d.height, &vopt, rgb.data(),
                                      nullptr)) != RT_OK) {
        return fail("rt_denoise_var", rc);
      }
      ms_denoise = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td).count();
    } else if (a.denoise) {
      rt_denoise_opts dopt;
      memset(&dopt, 0, sizeof dopt);  // the library defaults
      dopt.demodulate = 1;
      auto td = std::chrono::steady_clock::now();
      if (a.split_emitters) {
        if ((rc = rt_denoise_emit(rgb.data(), &f, &fe, d.width, d.height, &dopt, rgb.data())) != RT_OK)
          return fail("rt_denoise_emit", rc);
      } else if ((rc = rt_denoise(rgb.data(), &f, d.width, d.height, &dopt, rgb.data())) != RT_OK) {
        return fail("rt_denoise", rc);
      }
      ms_denoise = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - td).count();
    }
    if (!a.aov.empty()) {
      float dmax = 0.0f;
      for (float v : depth) dmax = v > dmax ? v : dmax;
      std::vector<float> nimg(3 * np), dimg(3 * np);
      for (size_t i = 0; i < 3 * np; ++i) nimg[i] = normal[i] * 0.5f + 0.5f;
      for (size_t i = 0; i < np; ++i) dimg[3 * i] = dimg[3 * i + 1] = dimg[3 * i + 2] = dmax > 0 ? depth[i] / dmax : 0.0f;
      const std::pair<const char*, const std::vector<float>*> outs[] = {
          {"_albedo.ppm", &albedo}, {"_normal.ppm", &nimg}, {"_depth.ppm", &dimg}};
      for (const auto& e : outs) {
        const std::string path = a.aov + e.first;
        if (write_ppm(*e.second, d.width, d.height, fopen(path.c_str(), "wb"), path.c_str())) return 1;
      }
      if (a.split_emitters) {  // the emission as it is, the coverage as grey
        std::vector<float> cimg(3 * np);
        for (size_t i = 0; i < np; ++i) cimg[3 * i] = cimg[3 * i + 1] = cimg[3 * i + 2] = coverage[i];
        const std::pair<const char*, const std::vector<float>*> eouts[] = {{"_emission.ppm", &emission},
                                                                            {"_coverage.ppm", &cimg}};
        for (const auto& e : eouts) {
          const std::string path = a.aov + e.first;
          if (write_ppm(*e.second, d.width, d.height, fopen(path.c_str(), "wb"), path.c_str())) return 1;
        }
      }
      if (a.aov_media) {  // the scatter fraction as grey
        std::vector<float> simg(3 * np);
        for (size_t i = 0; i < np; ++i) simg[3 * i] = simg[3 * i + 1] = simg[3 * i + 2] = scatter[i];
        const std::string path = a.aov + "_scatter.ppm";
        if (write_ppm(simg, d.width, d.height, fopen(path.c_str(), "wb"), path.c_str())) return 1;
      }
    }
  }

  // camera.go:160 header + PrintColor per pixel, then main.go:477's single write
  if (write_ppm(rgb, d.width, d.height, out, out_name.c_str())) return 1;
  double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::string js = stats_json(st, d, scene, wall, aov_samples, ms_aov, ms_denoise, accumulate ? &ai : nullptr,
                              ms_accum, a.denoise_var, a.adaptive_set ? &adi : nullptr, a.split_emitters,
                              a.accum_features, numbered ? frame : -1, a.temporal, ms_reproject, a.temporal_emit,
                              a.aov_media);
  if (a.stats || a.denoise || a.denoise_var || a.temporal) fprintf(stderr, "%s\n", js.c_str());
  if (!a.cpuprofile.empty()) {
    FILE* p = fopen(a.cpuprofile.c_str(), "w");
    if (!p) {
      fprintf(stderr, "rtbench: cannot create %s\n", a.cpuprofile.c_str());
      return 1;
    }
    fprintf(p, "%s\n", js.c_str());
    fclose(p);
  }
  if (acc && (rc = rt_accum_destroy(acc)) != RT_OK) return fail("rt_accum_destroy", rc);
  }  // frames
  rt_scene_destroy(sc);
  rt_tree_destroy(tree);
  return 0;
}
