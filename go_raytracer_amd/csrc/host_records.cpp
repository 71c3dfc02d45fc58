// host_records.cpp — the traversal's leaf records and the record loop's pair layout, packed
// on the host from the flattened scene (no GPU needed): what upload_scene (rt_render.hip)
// copies to the device and rt_scene_export_records hands to the CPU tests.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "rt_internal.h"

namespace rt {

// the traversal's leaf records (rt_device.h "leaf records"), in refs order
void build_leaf_records(const HostScene& h, std::vector<F4>& recs) {
  recs.assign(4 * h.refs.size(), F4{0, 0, 0, 0});
  for (size_t i = 0; i < h.refs.size(); ++i) make_record(h, h.refs[i], &recs[4 * i]);
}
// light table entries: quad lights as leaf records with the area in [2].w (prim_pdf)
void build_light_records(const HostScene& h, std::vector<F4>& recs) {
  recs.assign(8 * std::max<size_t>(h.lights.size(), 1), F4{0, 0, 0, 0});
  for (size_t i = 0; i < h.lights.size(); ++i) {
    const uint32_t ref = h.lights[i].ref;
    if (ref == PRIM_NONE || (ref >> 30) != PRIM_QUAD) continue;
    make_record(h, ref, &recs[8 * i]);
    const F4* q = &h.quad[5 * (size_t)(ref & 0x3FFFFFFFu)];  // Q|D, u|area, v|mat, n, w
    recs[8 * i + 2].w = q[1].w;                                // area
    recs[8 * i + 4] = q[0];
    recs[8 * i + 5] = q[1];
    recs[8 * i + 6] = q[2];
  }
}
void make_record(const HostScene& h, uint32_t ref, F4* r) {
  const uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
  float rb;
  memcpy(&rb, &ref, 4);
  if (type == PRIM_SPHERE) {
    const F4 cr = h.sph_cr[idx], mv = h.sph_mv[idx];
    r[0] = {cr.x, cr.y, cr.z, rb};
    r[1] = {mv.x, mv.y, mv.z, cr.w};
  } else if (type == PRIM_BOX) {  // box leaf (rt_device.h), built by the flattener
    for (int k = 0; k < 4; ++k) r[k] = h.box_recs[4 * (size_t)idx + k];
    r[0].w = rb;
  } else if (type == PRIM_QUAD) {
    const F4* q = &h.quad[5 * (size_t)idx];  // Q|D, u|area, v|mat, n, w
    const double u[3] = {q[1].x, q[1].y, q[1].z}, v[3] = {q[2].x, q[2].y, q[2].z},
                 w[3] = {q[4].x, q[4].y, q[4].z};
    auto cr = [](const double* a, const double* b, int k) {
      return k == 0 ? a[1] * b[2] - a[2] * b[1] : k == 1 ? a[2] * b[0] - a[0] * b[2]
                                                         : a[0] * b[1] - a[1] * b[0];
    };
    r[0] = {q[0].x, q[0].y, q[0].z, rb};
    r[1] = {q[3].x, q[3].y, q[3].z, q[0].w};
    r[2] = {(float)cr(v, w, 0), (float)cr(v, w, 1), (float)cr(v, w, 2), 0.0f};
    r[3] = {(float)cr(w, u, 0), (float)cr(w, u, 1), (float)cr(w, u, 2), 0.0f};
  } else {
    const F4* t = &h.tri[3 * (size_t)idx];  // v0|mat, e0|area, e1|flags
    r[0] = {t[0].x, t[0].y, t[0].z, rb};
    r[1] = {t[1].x, t[1].y, t[1].z, 0.0f};
    r[2] = {t[2].x, t[2].y, t[2].z, 0.0f};
  }
}

// per-material "texture reads u,v" flag for sphere UV (stored in the pad)
std::vector<DevMaterial> materials_with_uv_flag(const HostScene& h) {
  std::vector<DevMaterial> mats = h.mats;
  for (auto& m : mats) {
    bool needs = false;
    std::vector<int> st;
    if (m.kind != RT_MAT_METAL && m.kind != RT_MAT_DIELECTRIC && m.tex >= 0) st.push_back(m.tex);
    int guard = 0;
    while (!st.empty() && guard++ < 4096) {
      int tx = st.back();
      st.pop_back();
      const DevTexture& T = h.texs[tx];
      if (T.kind == RT_TEX_IMAGE) needs = true;
      if (T.kind == RT_TEX_CHECKER) {
        st.push_back(T.a);
        st.push_back(T.b);
      }
    }
    m._pad = needs ? 1.0f : 0.0f;
  }
  return mats;
}

// the BVH2 and the record-loop pairs serve tiny scenes only (render_impl's tree
// choice: <= 64 leaf entries); a 1M-triangle scene would upload 64 MB of BVH2
bool tiny_scene(const HostScene& h) {
  const size_t tiny = (size_t)std::max(64, tune_int("RT_BRUTE_MAX", kBruteMax));
  return h.refs.size() <= tiny;
}

namespace {

// The scene's leaf records with the tests that sort them into the record loop's groups.
struct Records {
  const HostScene& h;
  std::vector<F4> recs;
  bool use_axis, use_vert;
  double area(uint32_t ref) const {
    const uint32_t type = ref >> 30, idx = ref & 0x3FFFFFFFu;
    if (type == PRIM_QUAD) return h.quad[5 * (size_t)idx + 1].w;
    if (type == PRIM_TRI) return h.tri[3 * (size_t)idx + 1].w;
    const double r = h.sph_cr[idx].w;
    return 4.0 * 3.141592653589793 * r * r;
  }
  bool larger(size_t a, size_t b) const { return area(h.refs[a]) > area(h.refs[b]); }
  // Axis-aligned quads (unit normal +-e_a, A_a = B_a = 0 exactly: Cornell's walls,
  // floor, ceiling and box tops) go in per-axis pair groups after the general
  // pairs; the loop tests them with the in-plane terms only, bit-identical to the
  // general test (rt_records.h brute_axis).  An odd record of a group joins the
  // general list.  RT_BRUTE_AXIS=0 keeps every record general (A/B).
  int axis_of(size_t i) const {
    const F4* r = &recs[4 * i];
    if (!use_axis || (h.refs[i] >> 30) != PRIM_QUAD) return -1;
    const float n[3] = {r[1].x, r[1].y, r[1].z}, A[3] = {r[2].x, r[2].y, r[2].z},
                B[3] = {r[3].x, r[3].y, r[3].z};
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      if ((n[a] == 1.0f || n[a] == -1.0f) && n[b] == 0.0f && n[c] == 0.0f && A[a] == 0.0f &&
          B[a] == 0.0f)
        return a;
    }
    return -1;
  }
  // y-parallel quads (n_y = A_y = 0 and B = (0, B_y, 0) exactly: the sides of Cornell's
  // boxes rotated about y) go in a pair group between the general and the axis-aligned
  // ones (rt_records.h brute_vert: the general test without its exact-zero terms, images
  // bit-identical; C2 -1.6 % against RT_BRUTE_VERT=0, which keeps them general).
  int vert_of(size_t i) const {
    const F4* r = &recs[4 * i];
    if (!use_vert || (h.refs[i] >> 30) != PRIM_QUAD || axis_of(i) >= 0) return -1;
    const float n[3] = {r[1].x, r[1].y, r[1].z}, A[3] = {r[2].x, r[2].y, r[2].z},
                B[3] = {r[3].x, r[3].y, r[3].z};
    // y only (brute_vert<1>): RotateY is the reference's only rotation
    return n[1] == 0.0f && A[1] == 0.0f && B[0] == 0.0f && B[2] == 0.0f && B[1] != 0.0f ? 1 : -1;
  }
};

// Boxes rotated about y (NewBox objects.go:208-240 under RotateY / Translate,
// transformation.go:13-110; Cornell's two boxes): six quad records whose corners are
// the eight corners of one box with a horizontal top and bottom.  The loop tests each
// such box once, as three slabs in the box's own frame -- the reference's rotateY.Hit
// frame, where each face's quad test is t = (k - o'_a) / d'_a -- instead of its six
// records (rt_records.h brute_box).  The face records stay in the array (after the box
// descriptors) for the winner's u, v and ref.  RT_BRUTE_BOX=0 keeps them in the groups.
struct BoxRec { size_t face[6]; double C[3], ax[3], az[3], H; };
std::vector<BoxRec> find_boxes(const HostScene& h, const std::vector<size_t>& ord,
                               std::vector<char>& in_box) {
  std::vector<BoxRec> boxes;
  if (tune_int("RT_BRUTE_BOX", 1) == 0) return boxes;
  auto qd = [&](size_t i, int k, double* out) {  // k: 0 Q, 1 u, 2 v
    const F4& f = h.quad[5 * (size_t)(h.refs[i] & 0x3FFFFFFFu) + k];
    out[0] = f.x, out[1] = f.y, out[2] = f.z;
  };
  auto corners = [&](size_t i, double P[4][3]) {
    double Q[3], u[3], v[3];
    qd(i, 0, Q), qd(i, 1, u), qd(i, 2, v);
    for (int c = 0; c < 3; ++c) {
      P[0][c] = Q[c], P[1][c] = Q[c] + u[c], P[2][c] = Q[c] + v[c];
      P[3][c] = Q[c] + u[c] + v[c];
    }
  };
  std::vector<size_t> quads;
  for (size_t i : ord)
    if ((h.refs[i] >> 30) == PRIM_QUAD) quads.push_back(i);
  // four corners of quad i == the four points F (as sets, within tol)
  auto same_face = [&](size_t i, const double F[4][3], double tol) {
    double P[4][3];
    corners(i, P);
    bool used[4] = {false, false, false, false};
    for (int a = 0; a < 4; ++a) {
      int m = -1;
      for (int b = 0; b < 4 && m < 0; ++b)
        if (!used[b] && fabs(P[a][0] - F[b][0]) <= tol && fabs(P[a][1] - F[b][1]) <= tol &&
            fabs(P[a][2] - F[b][2]) <= tol)
          m = b;
      if (m < 0) return false;
      used[m] = true;
    }
    return true;
  };
  for (size_t i : quads) {
    if (in_box[i]) continue;
    double C[3], ax[3], az[3];
    qd(i, 0, C), qd(i, 1, ax), qd(i, 2, az);
    const double la = sqrt(ax[0] * ax[0] + ax[2] * ax[2]), lb = sqrt(az[0] * az[0] + az[2] * az[2]);
    // a horizontal rectangle: the bottom (or top) face of a candidate box
    if (ax[1] != 0.0 || az[1] != 0.0 || la == 0.0 || lb == 0.0 ||
        fabs(ax[0] * az[0] + ax[2] * az[2]) > 1e-6 * la * lb)
      continue;
    const double tol = 1e-5 * (1.0 + fabs(C[0]) + fabs(C[1]) + fabs(C[2]) + la + lb);
    auto corner = [&](int k, double H, double* out) {  // bit 0: +ax, 1: +az, 2: +H
      for (int c = 0; c < 3; ++c)
        out[c] = C[c] + ((k & 1) ? ax[c] : 0.0) + ((k & 2) ? az[c] : 0.0) + (c == 1 && (k & 4) ? H : 0.0);
    };
    // faces by (axis, side): x' = bit 0, y = bit 2, z' = bit 1
    const int fbit[3] = {1, 4, 2};
    for (size_t j : quads) {
      if (j == i || in_box[j]) continue;
      double Qj[3];
      qd(j, 0, Qj);
      const double H = Qj[1] - C[1];
      if (fabs(H) <= tol) continue;
      BoxRec b{};
      bool ok = true;
      for (int f = 0; f < 6 && ok; ++f) {
        double F[4][3];
        int n = 0;
        for (int k = 0; k < 8; ++k)
          if (((k & fbit[f >> 1]) != 0) == (f & 1)) corner(k, H, F[n++]);
        size_t hit = (size_t)-1;
        if (f == 2) hit = i;
        else if (f == 3) hit = same_face(j, F, tol) ? j : (size_t)-1;
        else
          for (size_t m : quads)
            if (m != i && m != j && !in_box[m] && same_face(m, F, tol)) {
              bool dup = false;
              for (int g = 0; g < f; ++g) dup |= b.face[g] == m;
              if (!dup) { hit = m; break; }
            }
        if (hit == (size_t)-1) ok = false;
        else b.face[f] = hit;
      }
      if (!ok) continue;
      for (int c = 0; c < 3; ++c) b.C[c] = C[c], b.ax[c] = ax[c], b.az[c] = az[c];
      b.H = H;
      for (int f = 0; f < 6; ++f) in_box[b.face[f]] = 1;
      boxes.push_back(b);
      break;
    }
  }
  return boxes;
}

struct Groups {
  std::vector<size_t> grp[7];  // 0-2: axis-aligned groups, 3: general, 4-6: axis-parallel
  std::vector<std::pair<int, size_t>> odd_ax;  // (axis, record): the mixed pair's halves, or empty
};
Groups group_records(const Records& R, const std::vector<size_t>& ord, const std::vector<char>& in_box) {
  Groups g;
  auto& grp = g.grp;
  auto& odd_ax = g.odd_ax;
  for (size_t i : ord) {
    if (in_box[i]) continue;
    const int a = R.axis_of(i);
    const int v = a < 0 ? R.vert_of(i) : -1;
    grp[a >= 0 ? a : v >= 0 ? 4 + v : 3].push_back(i);
  }
  // The odd records of two axis-aligned groups of different axes form one mixed pair, each
  // half tested on its own axis (rt_records.h brute_mixed: the axis test, bit for bit, ~35 VALU
  // where the general pair was ~85; Cornell's light and back wall).  Any other odd record
  // joins the general list.  (Padding each odd group with a never-hit record instead measured
  // 2.5 % slower on C2: one more loop and its per-axis setup.)  RT_BRUTE_MIXED=0: no mixed pair.
  for (int a : {0, 1, 2, 4, 5, 6})
    if (grp[a].size() & 1) {
      if (a < 3 && tune_int("RT_BRUTE_MIXED", 1) != 0) odd_ax.push_back({a, grp[a].back()});
      else grp[3].push_back(grp[a].back());  // the group's smallest record
      grp[a].pop_back();
    }
  if (odd_ax.size() == 3) {  // the third joins the general list
    grp[3].push_back(odd_ax.back().second);
    odd_ax.pop_back();
  }
  if (odd_ax.size() == 1) {
    grp[3].push_back(odd_ax.back().second);
    odd_ax.clear();
  }
  std::stable_sort(grp[3].begin(), grp[3].end(), [&](size_t a, size_t b) { return R.larger(a, b); });
  return g;
}

struct SlotOrder {
  std::vector<long> slots;  // record per slot in loop order, -1 = pad, -2 = box descriptor
  size_t n_general = 0;     // general and axis-parallel: the stored D
  size_t n_loop = 0;        // records the loop tests one by one
  size_t nbp = 0;           // box descriptor pairs
  size_t face0 = 0;         // first of the six face records per box
};
SlotOrder order_slots(const Groups& g, const std::vector<BoxRec>& boxes, BruteCounts& bc) {
  SlotOrder so;
  auto& slots = so.slots;
  for (size_t i : g.grp[3]) slots.push_back((long)i);
  if (slots.size() & 1) slots.push_back(-1);
  bc.ng = (int32_t)(slots.size() / 2);
  for (int a = 0; a < 3; ++a)
    for (size_t i : g.grp[4 + a]) slots.push_back((long)i);
  bc.vy = (int32_t)(g.grp[5].size() / 2);  // (only y is grouped: vert_of)
  so.n_general = slots.size();
  for (int a = 0; a < 3; ++a) {
    for (size_t i : g.grp[a]) slots.push_back((long)i);
    bc.ax[a] = (int32_t)(g.grp[a].size() / 2);
  }
  bc.mx = 0;  // the mixed pair (axes a0 < a1): (a0 + 1) | (a1 + 1) << 2
  if (g.odd_ax.size() == 2) {
    slots.push_back((long)g.odd_ax[0].second);  // odd_ax is in axis order (0, 1, 2 above)
    slots.push_back((long)g.odd_ax[1].second);
    bc.mx = (g.odd_ax[0].first + 1) | ((g.odd_ax[1].first + 1) << 2);
  }
  so.n_loop = slots.size();
  // box descriptors, two per pair slot (an odd box count repeats the last box: the
  // same t and faces, so the winner is unchanged), then the six face records per box
  so.nbp = (boxes.size() + 1) / 2;
  bc.box = (int32_t)so.nbp;
  slots.insert(slots.end(), 2 * so.nbp, -2);
  so.face0 = slots.size();
  for (const BoxRec& b : boxes)
    for (int f = 0; f < 6; ++f) slots.push_back((long)b.face[f]);
  if (slots.empty()) {
    slots.assign(2, -1);
    bc.ng = 1;
  }
  return so;
}

// pair layout (rt_device.h): records 2p, 2p+1 interleaved field by field
std::vector<F4> interleave_pairs(const Records& R, const SlotOrder& so, const std::vector<BoxRec>& boxes) {
  const auto& slots = so.slots;
  std::vector<F4> pairs(4 * slots.size(), F4{0, 0, 0, 0});  // pad: n = 0, never hit
  for (size_t k = 0; k < 2 * so.nbp; ++k) {
    // rt_records.h brute_box: C.x, C.z, ax/|ax|^2 (x, z), az/|az|^2 (x, z), y range, faces
    const BoxRec& b = boxes[std::min(k, boxes.size() - 1)];
    float* f = (float*)&pairs[4 * (so.n_loop + k - (k & 1))] + (k & 1);
    const double a2 = b.ax[0] * b.ax[0] + b.ax[2] * b.ax[2], z2 = b.az[0] * b.az[0] + b.az[2] * b.az[2];
    const double y0 = b.C[1], y1 = b.C[1] + b.H;
    const float v[8] = {(float)b.C[0], (float)b.C[2], (float)(b.ax[0] / a2), (float)(b.ax[2] / a2),
                        (float)(b.az[0] / z2), (float)(b.az[2] / z2), (float)std::min(y0, y1),
                        (float)std::max(y0, y1)};
    for (int e = 0; e < 8; ++e) f[2 * e] = v[e];
    for (int fc = 0; fc < 6; ++fc) {
      // face slot by (axis x' / y / z', low / high side); y's low side is the lower face
      const int src = (fc >> 1) == 1 && b.H < 0 ? (fc ^ 1) : fc;
      const uint32_t slot = (uint32_t)(so.face0 + 6 * std::min(k, boxes.size() - 1) + src);
      memcpy(&f[2 * (8 + fc)], &slot, 4);
    }
  }
  for (size_t i = 0; i < slots.size(); ++i) {
    if (slots[i] < 0) continue;
    const F4* r = &R.recs[4 * (size_t)slots[i]];  // Q|ref, n|D, A, B
    float* f = (float*)&pairs[8 * (i / 2)] + (i & 1);
    float kb;
    const uint32_t k = (uint32_t)i;
    memcpy(&kb, &k, 4);
    // axis records: D / n_a (= +-D exactly) in the D slot, so t = (D' - o_a) / d_a
    const int a = i >= so.n_general && i < so.n_loop ? R.axis_of((size_t)slots[i]) : -1;
    const float na = a == 0 ? r[1].x : a == 1 ? r[1].y : r[1].z;
    const float Dp = a < 0 ? r[1].w : na * r[1].w;
    const float v[15] = {r[1].x, r[1].y, r[1].z, Dp,     r[0].x, r[0].y, r[0].z, r[2].x,
                         r[2].y, r[2].z, r[3].x, r[3].y, r[3].z, kb,     r[0].w};
    for (int e = 0; e < 15; ++e) f[2 * e] = v[e];
  }
  return pairs;
}

// The lean set's shade table, after the pairs: per quad its normal and material kind,
// and its texture's solid colour (2 F4), so the record-loop kernel shades from LDS
// instead of three dependent global loads (quad, material, texture) per vertex, whose
// s_waitcnt vmcnt(0) also waited for the chunk flushes' pixel atomics
// (profiles/r4_phases_flush_c2.jsonl).  Only when every quad's material is Lambertian
// or a diffuse light with a solid texture (what the lean kernel shades).
std::vector<F4> shade_table(const HostScene& h) {
  const size_t nq = h.quad.size() / 5;
  std::vector<F4> tab(2 * nq);
  bool ok = nq > 0;
  for (size_t qi = 0; qi < nq && ok; ++qi) {
    const F4* q = &h.quad[5 * qi];
    uint32_t mb;
    memcpy(&mb, &q[2].w, 4);
    ok = mb < h.mats.size();
    if (!ok) break;
    const DevMaterial& m = h.mats[mb];
    ok = (m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT) && m.tex >= 0 &&
         (size_t)m.tex < h.texs.size() && h.texs[m.tex].kind == RT_TEX_SOLID;
    if (!ok) break;
    float kb;
    const uint32_t kind = (uint32_t)m.kind;
    memcpy(&kb, &kind, 4);
    tab[2 * qi] = {q[3].x, q[3].y, q[3].z, kb};
    // the colour, and the plane offset D (shade_core puts the hit point on the plane)
    const F4 col = h.texs[m.tex].color;
    tab[2 * qi + 1] = {col.x, col.y, col.z, q[0].w};
  }
  if (!ok || tune_int("RT_SHADE_LDS", 1) == 0) tab.clear();
  return tab;
}

// The lean kernel's early draw (rt_path.h shade_core<.., EARLY_SHAPE>) takes "the hit scatters" from
// the winning slot alone: true for every winner but the emitter slot.  That is the shade
// table's M.kind != RT_MAT_DIFFUSE_LIGHT exactly when the world has one emissive record, that
// record is the one quad light of a lean light kind, and it is tested as an ordinary record
// (a box code resolves to a face only after the draw, so no box face may be emissive).  Only
// the listed layouts have such a kernel.  -1: the scene is outside this.
int32_t emitter_slot_of(const HostScene& h, const SlotOrder& so, const std::vector<char>& in_box, int shape) {
  if (shape == 0 || lean_light_of(h, nullptr) != 1) return -1;
  auto mat_of = [](const F4* q) {
    uint32_t mb;
    memcpy(&mb, &q[2].w, 4);
    return mb;
  };
  long rec = -1;
  for (size_t i = 0; i < h.refs.size(); ++i) {
    if ((h.refs[i] >> 30) != PRIM_QUAD) return -1;
    const uint32_t mb = mat_of(&h.quad[5 * (size_t)(h.refs[i] & 0x3FFFFFFFu)]);
    if (mb >= h.mats.size()) return -1;
    if (h.mats[mb].kind != RT_MAT_DIFFUSE_LIGHT) continue;
    if (rec >= 0) return -1;  // a second emissive record
    rec = (long)i;
  }
  if (rec < 0 || in_box[(size_t)rec]) return -1;
  // the lights list holds its own copy of the quad (host_flatten.cpp walk_lights): the same
  // Q, u, v and material
  const F4* wq = &h.quad[5 * (size_t)(h.refs[(size_t)rec] & 0x3FFFFFFFu)];
  const F4* lq = &h.quad[5 * (size_t)(h.lights[0].ref & 0x3FFFFFFFu)];
  for (int k = 0; k < 3; ++k)
    if (!(wq[k].x == lq[k].x && wq[k].y == lq[k].y && wq[k].z == lq[k].z)) return -1;
  if (mat_of(wq) != mat_of(lq)) return -1;
  for (size_t k = 0; k < so.n_loop; ++k)
    if (so.slots[k] == rec) return (int32_t)k;
  return -1;
}

}  // namespace

RecordPack pack_records(const HostScene& h) {
  RecordPack out;
  if (!tiny_scene(h)) return out;
  Records R{h, {}, tune_int("RT_BRUTE_AXIS", 1) != 0, tune_int("RT_BRUTE_VERT", 1) != 0};
  build_leaf_records(h, R.recs);
  // record-loop order: largest surface first, so the closest hit tends to be found
  // early and later records fail the interval test before their slower half
  std::vector<size_t> ord(h.refs.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return R.larger(a, b); });
  std::vector<char> in_box(h.refs.size(), 0);
  const std::vector<BoxRec> boxes = find_boxes(h, ord, in_box);
  const Groups groups = group_records(R, ord, in_box);
  const SlotOrder so = order_slots(groups, boxes, out.counts);
  out.pairs = interleave_pairs(R, so, boxes);
  out.n_slots = so.slots.size();
  out.n_boxes = (int32_t)boxes.size();
  out.shape = brute_shape_of(out.counts);
  out.emitter_slot = emitter_slot_of(h, so, in_box, out.shape);
  const std::vector<F4> tab = shade_table(h);
  out.shade_n = (int32_t)tab.size();
  out.pairs.insert(out.pairs.end(), tab.begin(), tab.end());
  return out;
}

// the weight merge needs non-negative suffix products: every texture value (solid
// colours; image and noise values are >= 0 by construction) and metal albedo >= 0
// (the background is checked per render)
int32_t scene_merge_ok(const HostScene& h) {
  for (const auto& t : h.texs)
    if (t.kind == RT_TEX_SOLID && !(t.color.x >= 0.0f && t.color.y >= 0.0f && t.color.z >= 0.0f))
      return 0;
  for (const auto& m : h.mats)
    if (m.kind == RT_MAT_METAL && !(m.albedo.x >= 0.0f && m.albedo.y >= 0.0f && m.albedo.z >= 0.0f))
      return 0;
  return 1;
}
// mixture-pdf floor (rt_path.h): only when every light entry is a real prim; an entry of
// an empty HittableList has pdf 0 by the reference's rules, and its 0/0 NaNs are kept
float scene_pdf_floor(const HostScene& h) {
  if (h.lights.empty()) return 0.0f;
  for (const auto& e : h.lights)
    if (e.ref == PRIM_NONE) return 0.0f;
  return 1e-30f;
}

// The lean kernel's light kind (rt_device.h "lean light kinds"): what the kernel compiled
// for a kind leaves out must be an exact no-op for this scene -- one entry (no search, no
// loop), a quad (no dispatch), weight 1.0f (no multiply), the normal on the kind's axis with
// A_a = B_a = 0 exactly (pack_records' axis test: the dropped terms are exact zeros), merge_ok
// and the pdf floor at the constants the kernel holds.  The block is copied from the light's
// record (build_light_records), D' as interleave_pairs stores it for an axis record.
int lean_light_of(const HostScene& h, LeanLight* block) {
  if (block) *block = LeanLight{};
  if (pick_ft_set(h.features) != 0u || h.lights.size() != 1) return 0;
  const DevLight& e = h.lights[0];
  if (e.ref == PRIM_NONE || (e.ref >> 30) != PRIM_QUAD || e.weight != 1.0f) return 0;
  if (scene_merge_ok(h) != 1 || scene_pdf_floor(h) != 1e-30f) return 0;
  std::vector<F4> lr;
  build_light_records(h, lr);  // [0..3] Q|ref, n|D, A|area, B ; [4..6] Q, u, v
  const float n[3] = {lr[1].x, lr[1].y, lr[1].z}, Q[3] = {lr[0].x, lr[0].y, lr[0].z},
              A[3] = {lr[2].x, lr[2].y, lr[2].z}, B[3] = {lr[3].x, lr[3].y, lr[3].z};
  for (int kind = 1; kind < kLeanLightCount; ++kind) {
    const int a = lean_light_axis(kind);
    if (a < 0) continue;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    if (!((n[a] == 1.0f || n[a] == -1.0f) && n[b] == 0.0f && n[c] == 0.0f && A[a] == 0.0f &&
          B[a] == 0.0f))
      continue;
    if (block) {
      const float f[kLeanLightFloats] = {
          Q[0],    Q[1],    Q[2],    n[a] * lr[1].w, A[0],    A[1],    A[2],    lr[2].w, B[0],    B[1],
          B[2],    0.0f,    lr[5].x, lr[5].y,        lr[5].z, 0.0f,    lr[6].x, lr[6].y, lr[6].z, 0.0f};
      memcpy(block->f, f, sizeof f);
    }
    return kind;
  }
  return 0;
}

}  // namespace rt
