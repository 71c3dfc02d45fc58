// rtbench: the reference's command line (main.go:414-478) over the C ABI, and the ABI's one C client.
//
//   rtbench [-o image.ppm] [-N cores] [-S scene] [-cpuprofile file] [extensions]
//
// main.go's flags with Go's flag-package syntax and exits (usage + 2, -h 0); the output file is
// created before anything renders and the default scene leaves it empty.  -h lists every flag
// and README.md describes the extensions.  main() parses, validates (make_job), opens the output
// and builds the scene (rt_tree_*, rt_demo_scene, rt_camera_derive, rt_scene_create); then every
// frame goes through the stages:
//
//   begin_frame     the frame's file names, its output file, the -orbit camera (no ABI call)
//   render          rt_render, or an accumulator: rt_accum_create, rt_accum_set_features, per pass
//                   rt_accum_add or rt_accum_select + rt_accum_add_active, rt_accum_info_get,
//                   rt_accum_resolve, rt_accum_adapt_info, rt_accum_counts; rt_progress on a thread
//   feature_planes  rt_render_aov[_emit|_media] or rt_accum_resolve_aov[_media]
//   temporal_step   rt_reproject[_emit | _light | _moments | _clip] (the host entries: this client links no HIP runtime)
//   filter          rt_denoise[_var][_emit]
//   write_aovs      rt_format_ppm per plane
//                   (-shares N: N accumulators, rt_accum_add_shares per pass, rt_pipeline_push_shares below)
//   pipeline_step   -on-device: rt_pipeline_push + rt_pipeline_ppm in place of the three stages above (the
//                   frame stays on the device; what comes back is the image's text)
//   finish_frame    rt_format_ppm, the statistics line (-cpuprofile has no pprof to drive on the
//                   GPU path: the file receives the same line), rt_accum_destroy
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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
  bool accum_features = false, temporal = false, temporal_emit = false, aov_media = false, aov_specular = false;
  bool temporal_light = false, temporal_moments = false, temporal_clip = false, temporal_specular = false;
  bool on_device = false;
  double clip_gamma = 0.0;
  long long frames = 0, spec_bounces = 0, moments_radius = 0;
  double moments_frames = 0.0;
  double spec_fuzz = 0.0;
  double orbit = 0.0;
  long long shares = 0;
  std::string devices;  // -devices a,b,...
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
      {"aov-specular", "with -aov, -denoise or -denoise-var: follow mirrors and glass in the feature buffers (first diffuse-hit guides, see -spec-bounces and -spec-fuzz); -aov also writes PREFIX_bounces.ppm",
       Flag::BOOL, &a.aov_specular, ""},
      {"aov", "write PREFIX_albedo.ppm, PREFIX_normal.ppm and PREFIX_depth.ppm (first-hit feature buffers)",
       Flag::STR, &a.aov, ""},
      {"assets", "directory holding earthmap.jpg / dragon.obj (default: <exe dir>/../assets)",
       Flag::STR, &a.assets, ""},
      {"clip-gamma", "with -temporal-clip: the box is mean +- G sigma per channel (0 = the library's default; finite, >= 0)",
       Flag::F64, &a.clip_gamma, "0"},
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
      {"devices", "with -shares N: the N devices the shares run on, a,b,... (a device may repeat); default: share i on device i % the device count",
       Flag::STR, &a.devices, ""},
      {"frames", "render N frames, frame k to the -o name with _00k before the extension (see -orbit)", Flag::INT,
       &a.frames, "0"},
      {"mode", "kernel strategy: auto, fused or wavefront", Flag::STR, &a.mode, "auto"},
      {"moments-frames", "with -temporal-moments: the history length in frames from which the moments are trusted (0 = 4; at least 2)",
       Flag::F64, &a.moments_frames, "0"},
      {"moments-radius", "with -temporal-moments: the radius of the window for shorter histories (0 = 3, a 7 x 7 window; -1 = no window; at most 8)",
       Flag::INT, &a.moments_radius, "0"},
      {"o", "Specify a custom output file", Flag::STR, &a.out, "image.ppm"},
      {"on-device", "with -accum-features and -passes / -until / -adaptive: keep the frame on the device: the temporal stage, the filter and the image's text go through one rt_pipeline (rt_pipeline_push, rt_pipeline_ppm) instead of the host entries; the files are the same bytes; not with -aov-media",
       Flag::BOOL, &a.on_device, ""},
      {"orbit", "with -frames: turn the camera's look_from about the vup axis through look_at by DEG degrees per frame",
       Flag::F64, &a.orbit, "0"},
      {"passes", "render N passes of -spp samples each (seeds seed .. seed+N-1) and write their exact mean",
       Flag::INT, &a.passes, "0"},
      {"progress", "print render progress on stderr", Flag::BOOL, &a.progress, ""},
      {"seed", "render seed (Philox key)", Flag::U64, &a.seed, "1"},
      {"shares", "with -on-device and -passes: accumulate each frame as N row-interleaved shares (rt_accum_add_shares) and push them into the pipeline (rt_pipeline_push_shares); the files are the same bytes; not with -adaptive, -until, -aov or -counts",
       Flag::INT, &a.shares, "0"},
      {"slices", "progress granularity: launches per render (0 = 20 with -progress)", Flag::INT,
       &a.slices, "0"},
      {"spec-bounces", "with -aov-specular or -temporal-specular: the last vertex a specular chain may reach (0 = 8, at most 64)", Flag::INT,
       &a.spec_bounces, "0"},
      {"spec-fuzz", "with -aov-specular or -temporal-specular: follow metals up to this fuzz (0 = perfect mirrors only)", Flag::F64,
       &a.spec_fuzz, "0"},
      {"split-emitters", "with -denoise or -denoise-var: keep directly seen lights out of the filter (emission split); -aov also writes PREFIX_emission.ppm and PREFIX_coverage.ppm",
       Flag::BOOL, &a.split_emitters, ""},
      {"spp", "override Camera.SamplesPerPixel (0 = the scene's)", Flag::INT, &a.spp, "0"},
      {"stats", "print render statistics (JSON) on stderr", Flag::BOOL, &a.stats, ""},
      {"temporal", "with -accum-features and -passes / -until / -adaptive: blend each frame with the reprojected history of the frames before it (rt_reproject)",
       Flag::BOOL, &a.temporal, ""},
      {"temporal-clip", "with -temporal-moments: clamp the reprojected colour to the current frame's neighbourhood before the blend (rt_reproject_clip, see -clip-gamma), which overrules a stale reflection on metal or glass",
       Flag::BOOL, &a.temporal_clip, ""},
      {"temporal-emit", "as -temporal, with directly seen lights kept out of the history (rt_reproject_emit); needs -split-emitters too",
       Flag::BOOL, &a.temporal_emit, ""},
      {"temporal-light", "as -temporal-emit, with emission and coverage carried as history planes too and the blended planes handed to the split filter (rt_reproject_light); instead of -temporal / -temporal-emit",
       Flag::BOOL, &a.temporal_light, ""},
      {"temporal-moments", "with -temporal, -temporal-emit or -temporal-light: carry the second moment of luminance through the history and take the variance from it, or from a window of the frame (rt_reproject_moments); makes -denoise-var valid with -passes 1, e.g. -S 6 -passes 1 -accum-features -split-emitters -denoise-var -temporal-emit -temporal-moments -frames 8 -orbit 1",
       Flag::BOOL, &a.temporal_moments, ""},
      {"temporal-specular", "with -temporal-moments and -accum-features: look the history of mirrors up through the virtual point (rt_reproject_spec): the accumulator also keeps the specular chains' normal, depth and bounces (see -spec-bounces and -spec-fuzz), which stand in for the first hit's in the history; not with -aov-media",
       Flag::BOOL, &a.temporal_specular, ""},
      {"tree-seed", "seed of the scene builder's rand (main.go's math/rand)", Flag::U64,
       &a.tree_seed, "1"},
      {"until", "add passes until the image's relative standard error is <= E (at most -passes, default 1024)",
       Flag::F64, &a.until, "0"},
      {"width", "override Camera.Width (0 = the scene's)", Flag::INT, &a.width, "0"},
  };
}

void usage(const char* prog) {
  Args defaults;
  fprintf(stderr, "Usage of %s:\n", prog);
  for (const Flag& f : flags(defaults)) {
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

// every usage error: the message, the usage, exit code 2
int usage_error(const char* prog, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fprintf(stderr, "\n");
  usage(prog);
  return 2;
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
    if (name.empty() || name[0] == '-' || name[0] == '=') return usage_error(argv[0], "bad flag syntax: %s", s.c_str());
    size_t eq = name.find('=');
    if (eq != std::string::npos) val = name.substr(eq + 1), name = name.substr(0, eq), has_val = true;
    if (name == "h" || name == "help") {
      usage(argv[0]);
      return 0;
    }
    const Flag* f = nullptr;
    for (const Flag& c : fl)
      if (name == c.name) f = &c;
    if (!f) return usage_error(argv[0], "flag provided but not defined: -%s", name.c_str());
    if (f->kind == Flag::BOOL && !has_val) {
      val = "true";
    } else if (!has_val) {
      if (i + 1 >= argc) return usage_error(argv[0], "flag needs an argument: -%s", name.c_str());
      val = argv[++i];
    }
    if (!set_value(*f, val))
      return usage_error(argv[0], "invalid value \"%s\" for flag -%s: parse error", val.c_str(), name.c_str());
    if (name == "adaptive") a.adaptive_set = true;
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

// ---------------------------------------------------------------- the validated job ---
enum class Features { NONE, PASS, ACCUM };  // where the feature planes come from
enum class Filter { NONE, PLAIN, VAR };

// What the run does, fixed before the output file exists; the stages read this, not the flags.
struct Job {
  Args a;  // the plain values: names, seeds, sizes
  bool accumulate = false, adaptive = false, passes_ok = true;  // -passes / -until / -adaptive
  int32_t pass_cap = 0;
  Features source = Features::NONE;
  bool accum_features = false, emit = false, media = false;  // the planes beyond the guides
  bool specular = false;  // the guides are of the first diffuse hit (rt_render_aov_spec)
  Filter filter = Filter::NONE;
  bool temporal = false, temporal_emit = false, want_var = false;
  bool temporal_light = false;  // the temporal stage through rt_reproject_light
  bool temporal_moments = false;  // ... through rt_reproject_moments in the stage's mode
  bool temporal_clip = false;     // ... through rt_reproject_clip instead
  bool temporal_specular = false;  // ... through rt_reproject_spec, fed the accumulator's chain planes
  bool on_device = false;  // temporal_step, filter and the image's text through one rt_pipeline
  bool counts = false, aov = false, print_stats = false;
  bool numbered = false;  // -frames: frame k goes to the -o name with _00k before the extension
  int n_frames = 1;
  int shares = 0;            // -shares: the frame's accumulator is this many row shares (0: one whole accumulator)
  std::vector<int> devices;  // -devices: the shares' devices (empty: share i on device i % the device count)
};

// -devices: "a,b,..." as non-negative integers; false for anything else
bool parse_devices(const std::string& text, std::vector<int>& out) {
  out.clear();
  size_t at = 0;
  while (at <= text.size()) {
    const size_t end = std::min(text.find(',', at), text.size());
    if (end == at || end - at > 4) return false;
    int v = 0;
    for (size_t i = at; i < end; ++i) {
      if (text[i] < '0' || text[i] > '9') return false;
      v = 10 * v + (text[i] - '0');
    }
    out.push_back(v);
    at = end + 1;
  }
  return true;
}

// the "flag X needs flag Y" checks in their precedence: the first that fails is reported.
// Returns the exit code, or -1 with `j` filled.
int make_job(const Args& a, const char* prog, Job& j) {
  const bool acc = a.passes > 0 || a.until > 0.0 || a.adaptive_set, filtered = a.denoise || a.denoise_var;
  std::vector<int> devices;
  const bool devices_ok = a.devices.empty() || parse_devices(a.devices, devices);
  const struct { bool bad; const char* msg; } checks[] = {
      {a.adaptive_set && !(a.adaptive > 0.0), "invalid value for flag -adaptive: the error threshold must be > 0"},
      {!a.counts.empty() && !a.adaptive_set, "-counts needs -adaptive"},
      // the variance comes from the passes: one pass has none
      // -temporal-moments modifies one of the three temporal stages
      {a.temporal_moments && !(a.temporal || a.temporal_emit || a.temporal_light),
       "-temporal-moments needs -temporal, -temporal-emit or -temporal-light"},
      {(a.moments_frames != 0.0 || a.moments_radius != 0) && !a.temporal_moments,
       "-moments-frames and -moments-radius need -temporal-moments"},
      {a.moments_radius < -1 || a.moments_radius > 8 || !(a.moments_frames >= 0.0) || !(a.moments_frames <= 3.0e38) ||
           (a.moments_frames > 0.0 && a.moments_frames < 2.0),
       "invalid value for flag -moments-radius (-1..8) / -moments-frames (0, or finite and >= 2)"},
      // -temporal-clip modifies -temporal-moments, and needs its window
      {a.temporal_clip && !a.temporal_moments, "-temporal-clip needs -temporal-moments"},
      {a.clip_gamma != 0.0 && !a.temporal_clip, "-clip-gamma needs -temporal-clip"},
      {a.temporal_clip && a.moments_radius == -1, "-temporal-clip needs the window: -moments-radius -1 has none"},
      // (a positive G that rounds to 0 as a float would silently select the default)
      {!(a.clip_gamma >= 0.0) || !(a.clip_gamma <= 3.0e38) || (a.clip_gamma > 0.0 && (float)a.clip_gamma == 0.0f),
       "invalid value for flag -clip-gamma (0, or a finite positive float)"},
      // -temporal-specular modifies -temporal-moments, and its planes are the accumulator's
      {a.temporal_specular && !a.temporal_moments, "-temporal-specular needs -temporal-moments"},
      {a.temporal_specular && !a.accum_features, "-temporal-specular needs -accum-features"},
      {a.temporal_specular && a.aov_media, "-temporal-specular does not combine with -aov-media"},
      // ... unless the history brings one (-temporal-moments)
      {a.denoise_var && !(a.passes >= 2 || ((a.until > 0.0 || a.adaptive_set) && a.passes == 0) ||
                          (a.temporal_moments && a.passes == 1)),
       "-denoise-var needs -passes N with N >= 2, or -until / -adaptive"},
      {a.split_emitters && !filtered, "-split-emitters needs -denoise or -denoise-var"},  // nothing to split for
      {a.accum_features && !acc, "-accum-features needs -passes, -until or -adaptive"},  // no accumulator to keep them
      {a.temporal && !(a.accum_features && acc),  // no guides, no history
       "-temporal needs -accum-features and -passes, -until or -adaptive"},
      {a.temporal_emit && !(a.split_emitters && a.accum_features && acc),  // no emit planes
       "-temporal-emit needs -split-emitters, -accum-features and -passes, -until or -adaptive"},
      // the emit planes as -temporal-emit; a stage of its own, not a modifier of the two others
      {a.temporal_light && (!(a.split_emitters && a.accum_features && acc) || a.temporal || a.temporal_emit),
       "-temporal-light needs -split-emitters, -accum-features and -passes, -until or -adaptive, and neither -temporal "
       "nor -temporal-emit"},
      {a.aov_media && !(filtered || !a.aov.empty() || a.accum_features),  // no feature buffers
       "-aov-media needs -aov, -denoise, -denoise-var or -accum-features"},
      {a.aov_specular && !(filtered || !a.aov.empty()), "-aov-specular needs -aov, -denoise or -denoise-var"},
      // its own entry: no emit or media structure, and the accumulator keeps first-hit sums
      {a.aov_specular && a.aov_media, "-aov-specular does not combine with -aov-media"},
      {a.aov_specular && a.split_emitters, "-aov-specular does not combine with -split-emitters"},
      {a.aov_specular && a.accum_features, "-aov-specular does not combine with -accum-features"},
      {(a.spec_bounces != 0 || a.spec_fuzz != 0.0) && !(a.aov_specular || a.temporal_specular),
       "-spec-bounces and -spec-fuzz need -aov-specular or -temporal-specular"},
      {a.spec_bounces < 0 || a.spec_bounces > 64 || !(a.spec_fuzz >= 0.0) || !(a.spec_fuzz <= 3.0e38),
       "invalid value for flag -spec-bounces (0..64) / -spec-fuzz (finite, >= 0)"},
      // -on-device: the pipeline's frames are an accumulator's with feature planes (first-hit sums, no media)
      {a.on_device && !(a.accum_features && acc), "-on-device needs -accum-features and -passes, -until or -adaptive"},
      {a.on_device && a.aov_media, "-on-device does not combine with -aov-media"},
      {a.frames < 0 || a.frames > 999 || !(a.orbit == a.orbit), "invalid value for flag -frames (0..999) / -orbit"},
      // -shares: the pipeline is the one consumer of a frame held as shares
      {a.shares < 0 || a.shares > 4096, "invalid value for flag -shares (1..4096)"},
      {a.shares > 0 && !a.on_device, "-shares needs -on-device"},
      {!a.devices.empty() && a.shares == 0, "-devices needs -shares"},
      // (the selection and the error figure are one accumulator's)
      {a.shares > 0 && (a.adaptive_set || a.until > 0.0), "-shares does not combine with -adaptive or -until"},
      {a.shares > 0 && (!a.aov.empty() || !a.counts.empty()), "-shares does not combine with -aov or -counts"},
      {!devices_ok || (!a.devices.empty() && (long long)devices.size() != a.shares),
       "invalid value for flag -devices: one non-negative device number per share, a,b,..."},
  };
  for (const auto& c : checks)
    if (c.bad) return usage_error(prog, "%s", c.msg);
  j.a = a;
  j.accumulate = acc;
  j.adaptive = a.adaptive_set;
  j.passes_ok = !(a.passes < 0 || a.passes > 0x7FFFFFFF || !(a.until >= 0.0));  // reported once the scene is built
  j.pass_cap = (int32_t)(a.passes > 0 ? a.passes : 1024);
  j.temporal_emit = a.temporal_emit;
  j.temporal_light = a.temporal_light;
  j.temporal_moments = a.temporal_moments;
  j.temporal_clip = a.temporal_clip;
  j.temporal_specular = a.temporal_specular;
  j.temporal = a.temporal || a.temporal_emit || a.temporal_light;  // the same stage, through rt_reproject_emit / _light
  j.aov = !a.aov.empty();
  if (filtered || j.aov || j.temporal) j.source = a.accum_features ? Features::ACCUM : Features::PASS;
  j.accum_features = a.accum_features;
  j.emit = a.split_emitters;
  j.media = a.aov_media;
  j.specular = a.aov_specular;
  j.filter = a.denoise_var ? Filter::VAR : a.denoise ? Filter::PLAIN : Filter::NONE;
  j.want_var = a.denoise_var || j.temporal;
  j.on_device = a.on_device;
  j.counts = !a.counts.empty();
  j.print_stats = a.stats || filtered || j.temporal || a.on_device;
  j.numbered = a.frames > 0;
  j.n_frames = j.numbered ? (int)a.frames : 1;
  j.shares = (int)a.shares;
  j.devices = devices;
  return -1;
}

std::string frame_name(const std::string& name, int k, bool before_ext) {
  char tag[16];
  snprintf(tag, sizeof tag, "_%03d", k);
  const size_t slash = name.rfind('/'), dot = name.rfind('.');
  const bool ext = before_ext && dot != std::string::npos && (slash == std::string::npos || dot > slash);
  return ext ? name.substr(0, dot) + tag + name.substr(dot) : name + tag;
}

// ------------------------------------------------------------------- owned handles ---
struct Release {
  void operator()(rt_tree* p) const { rt_tree_destroy(p); }
  void operator()(rt_scene* p) const { rt_scene_destroy(p); }
  void operator()(rt_accum* p) const { rt_accum_destroy(p); }
  void operator()(rt_pipeline* p) const { rt_pipeline_destroy(p); }
  void operator()(FILE* p) const { fclose(p); }
};
template <class T>
using Owned = std::unique_ptr<T, Release>;

// the last ABI call's name and code, for the one failure report
struct Call {
  const char* what = "";
  int rc = RT_OK;
  bool ok(const char* name, int code) {
    what = name, rc = code;
    return code == RT_OK;
  }
};

int fail(const char* what, int rc) {
  fprintf(stderr, "rtbench: %s failed (%d): %s\n", what, rc, rt_last_error());
  return 1;
}

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The run and its current frame: what the stages work on.
struct Ctx {
  const char* scene = nullptr;
  rt_scene* sc = nullptr;
  rt_camera cam0, cam;  // the scene's camera, the frame's
  rt_camera_derived d;
  rt_render_opts o;
  std::chrono::steady_clock::time_point t0;
  int frame = 0;
  std::string out_name, aov;  // the frame's image and -aov prefix
  Owned<FILE> out;
  Owned<rt_accum> acc;
  std::vector<Owned<rt_accum>> shares;  // -shares: the frame's accumulators, rank i of shares.size()
  std::vector<rt_accum*> share_ptrs;
  std::vector<float> rgb, var, albedo, normal, depth, emission, salbedo, coverage, scatter, bounces;
  rt_stats st;
  rt_accum_info ai;
  rt_adapt_info adi;
  int aov_samples = 0;
  double ms_accum = 0.0, ms_aov = 0.0, ms_denoise = 0.0, ms_reproject = 0.0;
  // -temporal: the history (the frames before this one, reprojected and blended) and its camera
  std::vector<float> h_rgb, h_var, h_count, h_normal, h_depth, h_emission, h_coverage, count;
  std::vector<float> l_emission, l_coverage;  // -temporal-light: the blended light planes of this frame
  // -temporal-moments: the history's second moment of luminance, and the frame's result (rt_reproject_moments
  // never writes into the current frame's buffers)
  std::vector<float> h_lum2, m_rgb, m_var, m_count, m_lum2;
  // -temporal-specular: the frame's chain planes (the history keeps them in h_normal, h_depth and h_bounces)
  std::vector<float> s_normal, s_depth, s_bounces, h_bounces;
  rt_camera h_cam;
  bool have_history = false;
  // -on-device: the object that owns all of the above on the device, the frame's text and the time of both calls
  Owned<rt_pipeline> pipe;
  std::vector<char> text;
  double ms_pipeline = 0.0;

  size_t n_px() const { return (size_t)d.width * d.height; }
  int spp() const { return d.spp_sqrt * d.spp_sqrt; }
  rt_aov guides() { return {albedo.data(), normal.data(), depth.data(), nullptr}; }
  rt_aov_emit emit_planes() { return {emission.data(), salbedo.data(), coverage.data()}; }
};

// -progress: a line on stderr while the frame renders; joined when the scope ends
struct Progress {
  std::atomic<bool> rendering{true};
  std::atomic<int> pass_no{0};
  std::thread bar;
  Progress(const Job& j, const Ctx& c) {
    if (!j.a.progress) return;
    bar = std::thread([this, &j, &c] {
      uint64_t done = 0, total = 0;
      while (rendering.load()) {
        if (rt_progress(c.sc, &done, &total) == RT_OK && total) {
          if (j.accumulate)
            fprintf(stderr, "\rrendering %s: pass %d of %d, %5.1f%%", c.scene, pass_no.load() + 1, j.pass_cap,
                    100.0 * done / total);
          else
            fprintf(stderr, "\rrendering %s: %5.1f%%", c.scene, 100.0 * done / total);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
      }
    });
  }
  void stop() {
    rendering = false;
    if (bar.joinable()) bar.join();
  }
  ~Progress() { stop(); }
};

// ---------------------------------------------------------------------- statistics ---
struct Stats {
  const rt_stats* st;
  const rt_camera_derived* d;
  const char* scene;
  double wall_s, ms_aov, ms_denoise, ms_accum, ms_reproject;
  int aov_samples;
  const rt_accum_info* acc;    // -passes / -until / -adaptive, else null
  const rt_adapt_info* adapt;  // -adaptive, else null
  bool denoise_var, split_emitters, accum_features, temporal, temporal_emit, temporal_light, aov_media, aov_specular;
  bool temporal_moments, temporal_clip, temporal_specular;
  bool on_device;
  double ms_pipeline;
  int shares;  // -shares, else 0
  int frame;  // -frames, else -1
};

void appendf(std::string& s, const char* fmt, ...) {
  va_list ap, ap2;
  va_start(ap, fmt);
  va_copy(ap2, ap);
  const int n = vsnprintf(nullptr, 0, fmt, ap);
  va_end(ap);
  const size_t at = s.size();
  s.resize(at + (size_t)n + 1);
  vsnprintf(&s[at], (size_t)n + 1, fmt, ap2);
  va_end(ap2);
  s.resize(at + (size_t)n);
}

std::string stats_json(const Stats& s) {
  const rt_stats& st = *s.st;
  const rt_camera_derived& d = *s.d;
  const int spp = d.spp_sqrt * d.spp_sqrt;
  std::string b;
  appendf(b, "{\"scene\": \"%s\", \"width\": %d, \"height\": %d, \"spp\": %d, \"max_depth\": %d, ", s.scene, d.width,
          d.height, spp, d.max_depth);
  appendf(b, "\"samples\": %" PRIu64 ", \"segments\": %" PRIu64 ", \"ms_render\": %.3f, \"samples_per_s\": %.6g, ",
          st.samples, st.segments, st.ms_total, st.ms_total > 0 ? st.samples / (st.ms_total * 1e-3) : 0.0);
  appendf(b, "\"mode\": %d, \"tree_width\": %d, \"chunk_samples\": %d, ", st.mode, st.tree_width, st.chunk_samples);
  appendf(b, "\"aov_samples\": %d, \"ms_aov\": %.3f, \"ms_denoise\": %.3f, ", s.aov_samples, s.ms_aov, s.ms_denoise);
  if (s.acc)
    appendf(b, "\"passes\": %d, \"rel_error\": %.6g, \"ms_accum\": %.3f, ", s.acc->passes, s.acc->rel_error, s.ms_accum);
  if (s.acc && s.denoise_var) b += "\"denoise_var\": 1, ";
  if (s.acc && s.adapt)
    appendf(b, "\"active_last\": %" PRIu64 ", \"samples_total\": %" PRIu64 ", \"samples_full\": %" PRIu64 ", ",
            s.adapt->active_pixels, s.adapt->total_samples,
            (uint64_t)s.acc->passes * (uint64_t)spp * (uint64_t)d.width * (uint64_t)d.height);
  if (s.split_emitters) b += "\"split_emitters\": 1, ";
  if (s.accum_features) b += "\"accum_features\": 1, ";
  if (s.frame >= 0) appendf(b, "\"frame\": %d, ", s.frame);
  if (s.temporal) appendf(b, "\"temporal\": 1, \"ms_reproject\": %.3f, ", s.ms_reproject);
  if (s.temporal_emit) b += "\"temporal_emit\": 1, ";
  if (s.temporal_light) b += "\"temporal_light\": 1, ";
  if (s.temporal_moments) b += "\"temporal_moments\": 1, ";
  if (s.temporal_clip) b += "\"temporal_clip\": 1, ";
  if (s.temporal_specular) b += "\"temporal_specular\": 1, ";
  if (s.aov_media) b += "\"aov_media\": 1, ";
  if (s.aov_specular) b += "\"aov_specular\": 1, ";
  if (s.on_device) appendf(b, "\"on_device\": 1, \"ms_pipeline\": %.3f, ", s.ms_pipeline);
  if (s.shares > 0) appendf(b, "\"shares\": %d, ", s.shares);
  appendf(b, "\"wall_s\": %.3f}", s.wall_s);
  return b;
}

// ------------------------------------------------------------------------- writers ---
// one image through the PPM writer (camera.go:160 + PrintColor) into `path`; `f` is closed
int write_ppm(const std::vector<float>& img, int w, int h, Owned<FILE> f, const char* path) {
  int64_t n = rt_format_ppm(img.data(), w, h, nullptr, 0);
  std::vector<char> text((size_t)(n > 0 ? n : 0));
  if (n < 0 || rt_format_ppm(img.data(), w, h, text.data(), n) != n) return fail("rt_format_ppm", (int)n);
  if (!f || fwrite(text.data(), 1, text.size(), f.get()) != text.size() || fclose(f.release()) != 0) {
    fprintf(stderr, "rtbench: writing %s failed\n", path);
    return 1;
  }
  return 0;
}

int write_ppm(const std::vector<float>& img, const Ctx& c, const std::string& path) {
  return write_ppm(img, c.d.width, c.d.height, Owned<FILE>(fopen(path.c_str(), "wb")), path.c_str());
}

// a plane as a grey image, plane / scale (0 where the scale is not positive)
std::vector<float> grey(const std::vector<float>& plane, float scale) {
  std::vector<float> img(3 * plane.size());
  for (size_t i = 0; i < plane.size(); ++i) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = scale > 0 ? plane[i] / scale : 0.0f;
  return img;
}

// -------------------------------------------------------------------------- stages ---
// Every stage returns the exit code that ends the run, or 0 to go on.

// -orbit: look_from turned about the vup axis through look_at (Rodrigues' formula)
rt_camera orbit_camera(const rt_camera& cam0, double degrees) {
  rt_camera cam = cam0;
  double from[3] = {0, 0, 0}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0};
  if (cam0.positioned)
    for (int i = 0; i < 3; ++i) from[i] = cam0.look_from[i], at[i] = cam0.look_at[i], up[i] = cam0.vup[i];
  const double th = degrees * M_PI / 180.0, co = cos(th), si = sin(th);
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
  return cam;
}

// the frame's names, its output file (frame 0's exists already) and its camera
int begin_frame(const Job& j, Ctx& c, int frame) {
  c.frame = frame;
  c.aov_samples = 0;
  c.ms_accum = c.ms_aov = c.ms_denoise = c.ms_reproject = c.ms_pipeline = 0.0;
  c.out_name = j.numbered ? frame_name(j.a.out, frame, true) : j.a.out;
  c.aov = j.numbered && j.aov ? frame_name(j.a.aov, frame, false) : j.a.aov;
  if (frame > 0) c.out.reset(fopen(c.out_name.c_str(), "wb"));
  if (!c.out) {
    fprintf(stderr, "Error creating output file\n");
    return 1;
  }
  c.cam = j.numbered ? orbit_camera(c.cam0, j.a.orbit * (double)frame) : c.cam0;
  return 0;
}

// -passes / -until / -adaptive: passes into the accumulator until the cap, the target or no tile is left
void add_passes(const Job& j, Ctx& c, std::atomic<int>& pass_no, Call& s) {
  rt_adapt_opts ado;
  memset(&ado, 0, sizeof ado);  // the library defaults: tile 8, min_passes 4, lum_floor 1e-2
  ado.rel_error = j.a.adaptive;
  for (int32_t p = 0; p < j.pass_cap; ++p) {
    rt_stats sp;
    pass_no = p;
    if (j.adaptive) {  // the noisy tiles only (Accumulator.render_adaptive); every tile at first
      uint64_t n_active = 0;
      if (!s.ok("rt_accum_select", rt_accum_select(c.acc.get(), &ado, &n_active)) || n_active == 0) break;
      if (!s.ok("rt_accum_add_active", rt_accum_add_active(c.acc.get(), j.a.seed + (uint64_t)p, &sp))) break;
    } else if (j.shares) {  // one pass of every share, side by side
      if (!s.ok("rt_accum_add_shares",
                rt_accum_add_shares(c.share_ptrs.data(), (int32_t)c.share_ptrs.size(), j.a.seed + (uint64_t)p, &sp)))
        break;
    } else if (!s.ok("rt_accum_add", rt_accum_add(c.acc.get(), j.a.seed + (uint64_t)p, &sp))) {
      break;
    }
    const uint64_t samples = c.st.samples + sp.samples, segments = c.st.segments + sp.segments;
    const double ms = c.st.ms_total + sp.ms_total;
    c.st = sp;  // the last pass's, with the totals over the passes
    c.st.samples = samples;
    c.st.segments = segments;
    c.st.ms_total = ms;
    if (j.a.until > 0.0 && p >= 1 &&
        (!s.ok("rt_accum_info_get", rt_accum_info_get(c.acc.get(), &c.ai)) || c.ai.rel_error <= j.a.until))
      break;
  }
}

// the accumulator's mean (and variance), its figures, and -counts: the passes per pixel as grey, count / max
void resolve_passes(const Job& j, Ctx& c, Call& s, bool& counts_failed) {
  // -on-device: the mean stays where it is (rt_pipeline_push resolves it on the device)
  if (j.shares) {  // the figures of the statistics line are share 0's: a third of the rows, say, of the same image
    s.ok("rt_accum_info_get", rt_accum_info_get(c.share_ptrs[0], &c.ai));
    return;
  }
  if (s.ok("rt_accum_resolve", rt_accum_resolve(c.acc.get(), j.on_device ? nullptr : c.rgb.data(),
                                                j.want_var && !j.on_device ? c.var.data() : nullptr)))
    s.ok("rt_accum_resolve", rt_accum_info_get(c.acc.get(), &c.ai));
  if (s.rc != RT_OK || !j.adaptive) return;
  if (!s.ok("rt_accum_adapt_info", rt_accum_adapt_info(c.acc.get(), &c.adi)) || !j.counts) return;
  std::vector<int32_t> cnt(c.n_px());
  if (!s.ok("rt_accum_counts", rt_accum_counts(c.acc.get(), cnt.data()))) return;
  counts_failed = write_ppm(grey(std::vector<float>(cnt.begin(), cnt.end()), (float)c.adi.max_count), c, j.a.counts) != 0;
}

// the frame's image: one render, or the accumulator's mean over the passes
int render(const Job& j, Ctx& c) {
  c.rgb.assign(3 * c.n_px(), 0.0f);
  c.var.assign(j.want_var ? c.n_px() : 0, 0.0f);
  memset(&c.st, 0, sizeof c.st);
  memset(&c.ai, 0, sizeof c.ai);
  memset(&c.adi, 0, sizeof c.adi);
  Call s;
  const uint32_t planes = RT_ACCUM_FEAT_GUIDES | (j.emit ? RT_ACCUM_FEAT_EMIT : 0u) | (j.media ? RT_ACCUM_FEAT_MEDIA : 0u);
  const rt_aov_spec_opts chain = {(int32_t)j.a.spec_bounces, (float)j.a.spec_fuzz};
  // the frame's accumulators: the whole image's, or with -shares rank i of N on the share's device
  const int n_acc = !j.accumulate ? 0 : j.shares ? j.shares : 1;
  const int n_dev = j.shares && j.devices.empty() ? rt_device_count() : 0;
  for (int i = 0; i < n_acc; ++i) {
    rt_render_opts o = c.o;
    if (j.shares) {
      o.rank = i, o.nranks = j.shares;
      o.device = j.devices.empty() ? (n_dev > 0 ? i % n_dev : 0) : j.devices[i];
      o.progress_slices = 0;
    }
    rt_accum* acc = nullptr;
    if (!s.ok("rt_accum_create", rt_accum_create(c.sc, &c.cam, &o, j.pass_cap, &acc))) return fail(s.what, s.rc);
    if (j.shares)
      c.shares.emplace_back(acc), c.share_ptrs.push_back(acc);
    else
      c.acc.reset(acc);
    if (j.accum_features && j.temporal_specular) {
      if (!s.ok("rt_accum_set_features_spec", rt_accum_set_features_spec(acc, planes | RT_ACCUM_FEAT_SPEC, &chain)))
        return fail(s.what, s.rc);
    } else if (j.accum_features && !s.ok("rt_accum_set_features", rt_accum_set_features(acc, planes)))
      return fail(s.what, s.rc);
  }

  bool counts_failed = false;
  Progress bar(j, c);
  if (!j.accumulate) {
    s.ok("rt_render", rt_render(c.sc, &c.cam, &c.o, c.rgb.data(), &c.st));
  } else {
    const auto tp = std::chrono::steady_clock::now();
    add_passes(j, c, bar.pass_no, s);
    if (s.rc == RT_OK) resolve_passes(j, c, s, counts_failed);
    c.ms_accum = ms_since(tp);
  }
  bar.stop();
  if (j.a.progress && j.accumulate)
    fprintf(stderr, "\rrendering %s: %d passes, 100.0%%      \n", c.scene, c.ai.passes);
  else if (j.a.progress)
    fprintf(stderr, "\rrendering %s: 100.0%%\n", c.scene);
  if (s.rc != RT_OK) return fail(s.what, s.rc);
  return counts_failed ? 1 : 0;  // (reported by write_ppm)
}

// -denoise / -aov / -temporal: the feature planes of the same camera rays, from a feature pass at
// min(spp, 16) samples or from the accumulator (the guides of every pass the pixel took)
int feature_planes(const Job& j, Ctx& c) {
  if (j.source == Features::NONE || (j.on_device && !j.aov)) return 0;  // -on-device: only -aov reads them on the host
  const size_t np = c.n_px();
  c.albedo.assign(3 * np, 0.0f), c.normal.assign(3 * np, 0.0f), c.depth.assign(np, 0.0f);
  c.emission.assign(j.emit ? 3 * np : 0, 0.0f), c.salbedo.assign(j.emit ? 3 * np : 0, 0.0f);
  c.coverage.assign(j.emit ? np : 0, 0.0f), c.scatter.assign(j.media ? np : 0, 0.0f);
  c.bounces.assign(j.specular ? np : 0, 0.0f);
  const bool pass = j.source == Features::PASS;
  const int n = c.aov_samples = pass && c.spp() >= 16 ? 16 : c.spp();
  const rt_aov f = c.guides();
  const rt_aov_emit fe = c.emit_planes(), *split = j.emit ? &fe : nullptr;
  const rt_aov_media fm = {c.scatter.data()};
  const rt_aov_spec fs = {c.bounces.data()};
  const rt_aov_spec_opts so = {(int32_t)j.a.spec_bounces, (float)j.a.spec_fuzz};
  rt_stats sa;
  Call s;
  const auto ta = std::chrono::steady_clock::now();
  if (!pass && j.media)
    s.ok("rt_accum_resolve_aov_media", rt_accum_resolve_aov_media(c.acc.get(), &f, split, &fm));
  else if (!pass)
    s.ok("rt_accum_resolve_aov", rt_accum_resolve_aov(c.acc.get(), &f, split));
  else if (j.specular)  // (make_job: a feature pass, neither -split-emitters nor -aov-media)
    s.ok("rt_render_aov_spec", rt_render_aov_spec(c.sc, &c.cam, &c.o, n, &so, &f, &fs, &sa));
  else if (j.media)
    s.ok("rt_render_aov_media", rt_render_aov_media(c.sc, &c.cam, &c.o, n, &f, split, &fm, &sa));
  else if (j.emit)
    s.ok("rt_render_aov_emit", rt_render_aov_emit(c.sc, &c.cam, &c.o, n, &f, &fe, &sa));
  else
    s.ok("rt_render_aov", rt_render_aov(c.sc, &c.cam, &c.o, n, &f, &sa));
  if (s.rc == RT_OK && j.temporal_specular) {  // (make_job: the accumulator's) the history's planes, not the filter's
    c.s_normal.assign(3 * np, 0.0f), c.s_depth.assign(np, 0.0f), c.s_bounces.assign(np, 0.0f);
    const rt_aov fc = {nullptr, c.s_normal.data(), c.s_depth.data(), nullptr};
    const rt_aov_spec fb = {c.s_bounces.data()};
    s.ok("rt_accum_resolve_aov_spec", rt_accum_resolve_aov_spec(c.acc.get(), &fc, &fb));
  }
  c.ms_aov = ms_since(ta);
  return s.rc == RT_OK ? 0 : fail(s.what, s.rc);
}

// -temporal: the history into this frame's camera, then this frame as the new history
int temporal_step(const Job& j, Ctx& c) {
  if (!j.temporal || j.on_device) return 0;
  const auto tr = std::chrono::steady_clock::now();
  const int w = c.d.width, h = c.d.height;
  c.count.assign(c.n_px(), (float)c.ai.passes);
  if (j.temporal_light) c.l_emission = c.emission, c.l_coverage = c.coverage;  // the first frame's are its own
  if (j.temporal_moments) {
    // every frame, the first without a history (prev = NULL): its variance is the window's
    const size_t n = c.n_px();
    c.m_rgb.resize(3 * n), c.m_var.resize(n), c.m_count.resize(n), c.m_lum2.resize(n);
    const rt_frame prev = {c.h_rgb.data(), c.h_var.data(), c.h_count.data(), c.h_normal.data(), c.h_depth.data(), 0.0f, 0};
    // -temporal-specular: the chain's normal and depth in the first hit's place, in both frames
    const bool sp = j.temporal_specular;
    const rt_frame cur = {c.rgb.data(), c.var.data(), nullptr, sp ? c.s_normal.data() : c.normal.data(),
                          sp ? c.s_depth.data() : c.depth.data(), (float)c.ai.passes, 0};
    const rt_spec_planes chain = {c.h_bounces.data(), c.s_bounces.data()};
    const rt_frame res = {c.m_rgb.data(), c.m_var.data(), c.m_count.data(), nullptr, nullptr, 0.0f, 0};
    const rt_aov_emit prev_emit = {c.h_emission.data(), nullptr, c.h_coverage.data()};
    const rt_aov_emit cur_emit = {c.emission.data(), nullptr, c.coverage.data()};
    const rt_aov_emit res_emit = {c.l_emission.data(), nullptr, c.l_coverage.data()};
    const rt_moments_opts mo = {(float)j.a.moments_frames, (int32_t)j.a.moments_radius};
    const int mode = j.temporal_light ? RT_REPROJECT_LIGHT : j.temporal_emit ? RT_REPROJECT_EMIT : RT_REPROJECT_PLAIN;
    const bool hh = c.have_history;
    const rt_clip_opts co = {(float)j.a.clip_gamma};
    Call s;
    if (sp)
      s.ok("rt_reproject_spec",
           rt_reproject_spec(mode, hh ? &c.h_cam : nullptr, hh ? &prev : nullptr, hh ? &prev_emit : nullptr,
                             hh ? c.h_lum2.data() : nullptr, &c.cam, &cur, &cur_emit, w, h, nullptr, &mo,
                             j.temporal_clip ? &co : nullptr, &chain, &res, &res_emit, c.m_lum2.data()));
    else if (j.temporal_clip)
      s.ok("rt_reproject_clip",
           rt_reproject_clip(mode, hh ? &c.h_cam : nullptr, hh ? &prev : nullptr, hh ? &prev_emit : nullptr,
                             hh ? c.h_lum2.data() : nullptr, &c.cam, &cur, &cur_emit, w, h, nullptr, &mo, &co, &res,
                             &res_emit, c.m_lum2.data()));
    else
      s.ok("rt_reproject_moments",
           rt_reproject_moments(mode, hh ? &c.h_cam : nullptr, hh ? &prev : nullptr, hh ? &prev_emit : nullptr,
                                hh ? c.h_lum2.data() : nullptr, &c.cam, &cur, &cur_emit, w, h, nullptr, &mo, &res,
                                &res_emit, c.m_lum2.data()));
    if (s.rc != RT_OK) return fail(s.what, s.rc);
    c.rgb = c.m_rgb, c.var = c.m_var, c.count = c.m_count, c.h_lum2 = c.m_lum2;
  } else if (c.have_history) {
    const rt_frame prev = {c.h_rgb.data(), c.h_var.data(), c.h_count.data(), c.h_normal.data(), c.h_depth.data(), 0.0f, 0};
    const rt_frame cur = {c.rgb.data(), c.var.data(), nullptr, c.normal.data(), c.depth.data(), (float)c.ai.passes, 0};
    const rt_frame res = {c.rgb.data(), c.var.data(), c.count.data(), nullptr, nullptr, 0.0f, 0};
    const rt_aov_emit prev_emit = {c.h_emission.data(), nullptr, c.h_coverage.data()};
    const rt_aov_emit cur_emit = {c.emission.data(), nullptr, c.coverage.data()};
    const rt_aov_emit res_emit = {c.l_emission.data(), nullptr, c.l_coverage.data()};
    Call s;
    if (j.temporal_light)
      s.ok("rt_reproject_light",
           rt_reproject_light(&c.h_cam, &prev, &prev_emit, &c.cam, &cur, &cur_emit, w, h, nullptr, &res, &res_emit));
    else if (j.temporal_emit)
      s.ok("rt_reproject_emit",
           rt_reproject_emit(&c.h_cam, &prev, &prev_emit, &c.cam, &cur, &cur_emit, w, h, nullptr, &res));
    else
      s.ok("rt_reproject", rt_reproject(&c.h_cam, &prev, &c.cam, &cur, w, h, nullptr, &res));
    if (s.rc != RT_OK) return fail(s.what, s.rc);
  }
  c.h_rgb = c.rgb, c.h_var = c.var, c.h_count = c.count, c.h_normal = c.normal, c.h_depth = c.depth;
  if (j.temporal_specular) c.h_normal = c.s_normal, c.h_depth = c.s_depth, c.h_bounces = c.s_bounces;
  if (j.temporal_emit) c.h_emission = c.emission, c.h_coverage = c.coverage;
  if (j.temporal_light) c.h_emission = c.l_emission, c.h_coverage = c.l_coverage;
  c.h_cam = c.cam;
  c.have_history = true;
  c.ms_reproject = ms_since(tr);
  return 0;
}

// -denoise / -denoise-var, with -split-emitters their _emit entries; in place, the library's defaults
int filter(const Job& j, Ctx& c) {
  if (j.filter == Filter::NONE || j.on_device) return 0;
  const int w = c.d.width, h = c.d.height;
  const rt_aov f = c.guides();
  // -temporal-light: rgb was re-lit from the blended planes, so rgb - emission is the surface part
  // only with them
  const rt_aov_emit fe = j.temporal_light ? rt_aov_emit{c.l_emission.data(), c.salbedo.data(), c.l_coverage.data()}
                                          : c.emit_planes();
  float* rgb = c.rgb.data();
  rt_denoise_var_opts vopt;
  rt_denoise_opts dopt;
  memset(&vopt, 0, sizeof vopt);
  memset(&dopt, 0, sizeof dopt);
  vopt.demodulate = dopt.demodulate = 1;
  Call s;
  const auto td = std::chrono::steady_clock::now();
  if (j.filter == Filter::VAR && j.emit)
    s.ok("rt_denoise_var_emit", rt_denoise_var_emit(rgb, c.var.data(), &f, &fe, w, h, &vopt, rgb, nullptr));
  else if (j.filter == Filter::VAR)
    s.ok("rt_denoise_var", rt_denoise_var(rgb, c.var.data(), &f, w, h, &vopt, rgb, nullptr));
  else if (j.emit)
    s.ok("rt_denoise_emit", rt_denoise_emit(rgb, &f, &fe, w, h, &dopt, rgb));
  else
    s.ok("rt_denoise", rt_denoise(rgb, &f, w, h, &dopt, rgb));
  c.ms_denoise = ms_since(td);
  return s.rc == RT_OK ? 0 : fail(s.what, s.rc);
}

// -on-device: the object temporal_step and filter are restated in, with their options: the library's defaults,
// the filters demodulating
int make_pipeline(const Job& j, Ctx& c) {
  if (!j.on_device) return 0;
  rt_pipeline_opts po;
  memset(&po, 0, sizeof po);
  po.temporal = j.temporal;
  po.mode = j.temporal_light ? RT_REPROJECT_LIGHT : j.temporal_emit ? RT_REPROJECT_EMIT : RT_REPROJECT_PLAIN;
  po.moments = j.temporal_moments, po.clip = j.temporal_clip, po.specular = j.temporal_specular;
  po.mopts.min_frames = (float)j.a.moments_frames, po.mopts.radius = (int32_t)j.a.moments_radius;
  po.copts.gamma = (float)j.a.clip_gamma;
  po.filter = j.filter == Filter::VAR ? RT_PIPE_FILTER_VAR : j.filter == Filter::PLAIN ? RT_PIPE_FILTER_PLAIN : RT_PIPE_FILTER_NONE;
  po.split_emitters = j.emit;
  po.dopts.demodulate = po.vopts.demodulate = 1;
  rt_pipeline* p = nullptr;
  const int rc = rt_pipeline_create(&po, &p);
  if (rc != RT_OK) return fail("rt_pipeline_create", rc);
  c.pipe.reset(p);
  return 0;
}

// -on-device: the frame through the pipeline, and its text straight into the buffer the file is written from
int pipeline_step(const Job& j, Ctx& c) {
  if (!j.on_device) return 0;
  const auto tp = std::chrono::steady_clock::now();
  int rc = j.shares ? rt_pipeline_push_shares(c.pipe.get(), c.share_ptrs.data(), (int32_t)c.share_ptrs.size())
                    : rt_pipeline_push(c.pipe.get(), c.acc.get());
  if (rc != RT_OK) return fail(j.shares ? "rt_pipeline_push_shares" : "rt_pipeline_push", rc);
  const int64_t n = rt_pipeline_ppm(c.pipe.get(), nullptr, 0);
  c.text.resize((size_t)(n > 0 ? n : 0));
  if (n < 0 || rt_pipeline_ppm(c.pipe.get(), c.text.data(), n) != n) return fail("rt_pipeline_ppm", (int)n);
  c.ms_pipeline = ms_since(tp);
  return 0;
}

// -aov: PREFIX_albedo, _normal as n * 0.5 + 0.5, _depth over the image maximum; the emission as it
// is; coverage and scatter as grey, bounces over the image maximum
int write_aovs(const Job& j, const Ctx& c) {
  if (!j.aov) return 0;
  float dmax = 0.0f;
  for (float v : c.depth) dmax = v > dmax ? v : dmax;
  std::vector<float> nimg(c.normal.size());
  for (size_t i = 0; i < nimg.size(); ++i) nimg[i] = c.normal[i] * 0.5f + 0.5f;
  const auto put = [&](const char* suffix, const std::vector<float>& img) { return write_ppm(img, c, c.aov + suffix); };
  if (put("_albedo.ppm", c.albedo) || put("_normal.ppm", nimg) || put("_depth.ppm", grey(c.depth, dmax))) return 1;
  if (j.emit && (put("_emission.ppm", c.emission) || put("_coverage.ppm", grey(c.coverage, 1.0f)))) return 1;
  if (j.media && put("_scatter.ppm", grey(c.scatter, 1.0f))) return 1;
  float bmax = 0.0f;
  for (float v : c.bounces) bmax = v > bmax ? v : bmax;
  if (j.specular && put("_bounces.ppm", grey(c.bounces, bmax))) return 1;
  return 0;
}

// camera.go:160 header + PrintColor per pixel, then main.go:477's single write; the statistics
int finish_frame(const Job& j, Ctx& c) {
  if (j.on_device) {  // the text is there already
    Owned<FILE> f = std::move(c.out);
    if (!f || fwrite(c.text.data(), 1, c.text.size(), f.get()) != c.text.size() || fclose(f.release()) != 0) {
      fprintf(stderr, "rtbench: writing %s failed\n", c.out_name.c_str());
      return 1;
    }
  } else if (write_ppm(c.rgb, c.d.width, c.d.height, std::move(c.out), c.out_name.c_str())) {
    return 1;
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - c.t0).count();
  Stats s;
  s.st = &c.st, s.d = &c.d, s.scene = c.scene, s.wall_s = wall;
  s.ms_aov = c.ms_aov, s.ms_denoise = c.ms_denoise, s.ms_accum = c.ms_accum, s.ms_reproject = c.ms_reproject;
  s.aov_samples = c.aov_samples;
  s.acc = j.accumulate ? &c.ai : nullptr;
  s.adapt = j.adaptive ? &c.adi : nullptr;
  s.denoise_var = j.filter == Filter::VAR, s.split_emitters = j.emit, s.accum_features = j.accum_features;
  s.temporal = j.temporal, s.temporal_emit = j.temporal_emit, s.temporal_light = j.temporal_light, s.temporal_moments = j.temporal_moments, s.temporal_clip = j.temporal_clip, s.temporal_specular = j.temporal_specular, s.aov_media = j.media, s.aov_specular = j.specular;
  s.on_device = j.on_device, s.ms_pipeline = c.ms_pipeline;
  s.shares = j.shares;
  s.frame = j.numbered ? c.frame : -1;
  const std::string js = stats_json(s);
  if (j.print_stats) fprintf(stderr, "%s\n", js.c_str());
  if (!j.a.cpuprofile.empty()) {
    Owned<FILE> p(fopen(j.a.cpuprofile.c_str(), "w"));
    if (!p) {
      fprintf(stderr, "rtbench: cannot create %s\n", j.a.cpuprofile.c_str());
      return 1;
    }
    fprintf(p.get(), "%s\n", js.c_str());
  }
  int rc = c.acc ? rt_accum_destroy(c.acc.release()) : RT_OK;
  c.share_ptrs.clear();
  for (Owned<rt_accum>& sh : c.shares)
    if (const int r = rt_accum_destroy(sh.release()); rc == RT_OK) rc = r;
  c.shares.clear();
  return rc == RT_OK ? 0 : fail("rt_accum_destroy", rc);
}

// the scene function's tree, the camera with the overrides, the device scene
int build_scene(const Job& j, Ctx& c, Owned<rt_tree>& tree, Owned<rt_scene>& sc) {
  const Args& a = j.a;
  std::string assets = a.assets.empty() ? exe_dir() + "/../assets" : a.assets;
  if (a.assets.empty() && getenv("RT_ASSET_DIR")) assets = getenv("RT_ASSET_DIR");
  rt_tree* t = nullptr;
  Call s;
  if (!s.ok("rt_tree_create", rt_tree_create(&t))) return fail(s.what, s.rc);
  tree.reset(t);
  rt_tree_seed(t, a.tree_seed);
  rt_camera& cam = c.cam0;
  memset(&cam, 0, sizeof cam);
  int world = -1, lights = -1;
  if (!s.ok("rt_demo_scene", rt_demo_scene(t, c.scene, assets.c_str(), &cam, &world, &lights))) return fail(s.what, s.rc);
  cam.max_threads = (int32_t)a.N;
  if (a.width > 0) cam.width = (int32_t)a.width;
  if (a.spp > 0) cam.samples_per_pixel = (int32_t)a.spp;
  if (a.depth > 0) cam.max_depth = (int32_t)a.depth;
  if (!s.ok("rt_camera_derive", rt_camera_derive(&cam, &c.d))) return fail(s.what, s.rc);
  rt_scene* scene = nullptr;
  if (!s.ok("rt_scene_create", rt_scene_create(t, world, lights, &scene))) return fail(s.what, s.rc);
  sc.reset(scene);
  c.sc = scene;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Args a;
  Job j;
  int rc = parse(argc, argv, a);
  if (rc >= 0) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = make_job(a, argv[0], j)) >= 0) return rc;

  // main.go:434-439: the output file exists before anything renders
  Owned<FILE> out(fopen((j.numbered ? frame_name(a.out, 0, true) : a.out).c_str(), "wb"));
  if (!out) {
    fprintf(stderr, "Error creating output file\n");
    return 1;
  }
  const char* scene = nullptr;
  if (a.S < 1 || a.S > 8 || rt_demo_scene_name((int)a.S, &scene) != RT_OK || !scene)
    return 0;  // defaultScene (main.go:412-414): nothing rendered, empty file
  const int mode = a.mode == "auto" ? RT_MODE_AUTO : a.mode == "fused" ? RT_MODE_FUSED
                   : a.mode == "wavefront" ? RT_MODE_WAVEFRONT : -1;
  if (mode < 0) {
    fprintf(stderr, "invalid value \"%s\" for flag -mode\n", a.mode.c_str());
    return 2;
  }

  Owned<rt_tree> tree;
  Owned<rt_scene> sc;  // after the tree and before the context: the accumulator goes first, then the scene
  Ctx c;
  c.scene = scene;
  c.t0 = t0;
  c.out = std::move(out);
  if ((rc = build_scene(j, c, tree, sc)) != 0) return rc;
  if (!j.passes_ok) {
    fprintf(stderr, "invalid value for flag -passes / -until\n");
    return 2;
  }
  memset(&c.o, 0, sizeof c.o);
  c.o.seed = a.seed;
  c.o.device = (int32_t)a.device;
  c.o.nranks = 1;
  c.o.mode = mode;
  c.o.trace_pixel = -1;
  c.o.progress_slices = (int32_t)(a.slices > 0 ? a.slices : a.progress ? 20 : 0);
  if ((rc = make_pipeline(j, c)) != 0) return rc;

  for (int frame = 0; frame < j.n_frames; ++frame) {
    if ((rc = begin_frame(j, c, frame)) != 0) return rc;
    if ((rc = render(j, c)) != 0) return rc;
    if ((rc = feature_planes(j, c)) != 0) return rc;
    if ((rc = temporal_step(j, c)) != 0) return rc;
    if ((rc = filter(j, c)) != 0) return rc;
    if ((rc = pipeline_step(j, c)) != 0) return rc;
    if ((rc = write_aovs(j, c)) != 0) return rc;
    if ((rc = finish_frame(j, c)) != 0) return rc;
  }
  return 0;
}
