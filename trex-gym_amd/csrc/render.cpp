// Host side of the renderer: face planes of every hull group's convex hull, and the primitive table the ray kernel
// (render.hip) reads. Computed from the hull VERTICES - not from mesh faces - so that OBJ (trex_collide.urdf) and DAE
// (collisions_dir) models are treated alike and the picture is exactly the convex hull the contact generation uses.
#include <algorithm>
#include <cmath>
#include <map>
#include <utility>

#include "model.hpp"
#include "render.h"

namespace trex {

namespace {

struct V3 { double x, y, z; };
V3 sub(const V3 &a, const V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 cross(const V3 &a, const V3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double norm(const V3 &a) { return std::sqrt(dot(a, a)); }

struct Face { int a, b, c; V3 n; double d; bool alive; };   // outward unit normal n, plane n.x = d

Face make_face(const std::vector<V3> &p, int a, int b, int c) {
  V3 n = cross(sub(p[b], p[a]), sub(p[c], p[a]));
  const double l = norm(n);
  n = {n.x / l, n.y / l, n.z / l};
  return {a, b, c, n, dot(n, p[a]), true};
}

}  // namespace

// Incremental convex hull in f64 (points in index order), then the triangles of one plane merged: a triangle joins a
// face when its three vertices lie within `tol` of the face's plane. Each plane is the unit normal of the face's
// largest triangle with d = max over ALL points of n.x, so every point satisfies n.x <= d exactly. A set with fewer
// than 4 non-coplanar points has no interior and yields no plane (it draws nothing).
std::vector<std::array<double, 4>> convex_hull_planes(const std::vector<Vec3> &pts_in) {
  std::vector<std::array<double, 4>> out;
  const int n = (int)pts_in.size();
  if (n < 4) return out;
  std::vector<V3> p(n);
  for (int i = 0; i < n; i++) p[i] = {pts_in[i].x, pts_in[i].y, pts_in[i].z};
  V3 lo = p[0], hi = p[0];
  for (auto &q : p) {
    lo = {std::min(lo.x, q.x), std::min(lo.y, q.y), std::min(lo.z, q.z)};
    hi = {std::max(hi.x, q.x), std::max(hi.y, q.y), std::max(hi.z, q.z)};
  }
  const double scale = std::max({hi.x - lo.x, hi.y - lo.y, hi.z - lo.z});
  if (!(scale > 0)) return out;
  const double eps = 1e-12 * scale;    // visibility: a point this close to a face's plane is on it
  const double tol = 1e-10 * scale;    // merge: triangles this close to one plane are one face
  // initial tetrahedron from extreme points
  int i0 = 0;
  for (int i = 1; i < n; i++) if (p[i].x < p[i0].x) i0 = i;
  int i1 = -1; double best = 0;
  for (int i = 0; i < n; i++) { double d = norm(sub(p[i], p[i0])); if (d > best) { best = d; i1 = i; } }
  if (i1 < 0 || best <= 1e-9 * scale) return out;
  int i2 = -1; best = 0;
  for (int i = 0; i < n; i++) { double d = norm(cross(sub(p[i1], p[i0]), sub(p[i], p[i0]))); if (d > best) { best = d; i2 = i; } }
  if (i2 < 0 || best <= 1e-9 * scale * scale) return out;
  const V3 n012 = cross(sub(p[i1], p[i0]), sub(p[i2], p[i0]));
  int i3 = -1; best = 0;
  for (int i = 0; i < n; i++) { double d = std::fabs(dot(n012, sub(p[i], p[i0]))) / norm(n012); if (d > best) { best = d; i3 = i; } }
  if (i3 < 0 || best <= 1e-9 * scale) return out;   // all points (nearly) coplanar
  std::vector<Face> faces;
  {
    int t[4] = {i0, i1, i2, i3};
    V3 ctr = {0, 0, 0};
    for (int k : t) ctr = {ctr.x + 0.25 * p[k].x, ctr.y + 0.25 * p[k].y, ctr.z + 0.25 * p[k].z};
    const int tri[4][3] = {{i0, i1, i2}, {i0, i3, i1}, {i0, i2, i3}, {i1, i3, i2}};
    for (auto &f : tri) {
      Face fc = make_face(p, f[0], f[1], f[2]);
      if (dot(fc.n, ctr) > fc.d) fc = make_face(p, f[0], f[2], f[1]);   // outward
      faces.push_back(fc);
    }
  }
  std::map<std::pair<int, int>, int> edges;   // directed edge -> owning face (of the visible set)
  for (int i = 0; i < n; i++) {
    if (i == i0 || i == i1 || i == i2 || i == i3) continue;
    std::vector<int> vis;
    for (int f = 0; f < (int)faces.size(); f++)
      if (faces[f].alive && dot(faces[f].n, p[i]) - faces[f].d > eps) vis.push_back(f);
    if (vis.empty()) continue;
    edges.clear();
    for (int f : vis) {
      const Face &F = faces[f];
      edges[{F.a, F.b}] = f; edges[{F.b, F.c}] = f; edges[{F.c, F.a}] = f;
    }
    std::vector<std::pair<int, int>> horizon;
    for (auto &e : edges)
      if (!edges.count({e.first.second, e.first.first})) horizon.push_back(e.first);
    for (int f : vis) faces[f].alive = false;
    for (auto &h : horizon) faces.push_back(make_face(p, h.first, h.second, i));
  }
  // merge the triangles of one plane
  std::vector<int> alive;
  for (int f = 0; f < (int)faces.size(); f++) if (faces[f].alive) alive.push_back(f);
  std::vector<bool> used(faces.size(), false);
  for (int f : alive) {
    if (used[f]) continue;
    const Face &F = faces[f];
    int bestf = f;
    double best_area = norm(cross(sub(p[F.b], p[F.a]), sub(p[F.c], p[F.a])));
    used[f] = true;
    for (int g : alive) {
      if (used[g]) continue;
      const Face &G = faces[g];
      if (dot(G.n, F.n) > 0 && std::fabs(dot(F.n, p[G.a]) - F.d) <= tol && std::fabs(dot(F.n, p[G.b]) - F.d) <= tol &&
          std::fabs(dot(F.n, p[G.c]) - F.d) <= tol) {
        used[g] = true;
        const double area = norm(cross(sub(p[G.b], p[G.a]), sub(p[G.c], p[G.a])));
        if (area > best_area) { best_area = area; bestf = g; }
      }
    }
    const V3 nn = faces[bestf].n;
    double d = -1e300;
    for (auto &q : p) d = std::max(d, dot(nn, q));
    out.push_back({nn.x, nn.y, nn.z, d});
  }
  return out;
}

void hull_group_planes(const HostModel &m, std::vector<double> &plane, std::vector<int> &start) {
  plane.clear();
  start.assign(1, 0);
  for (size_t g = 0; g + 1 < m.hull_group_start.size(); g++) {
    std::vector<Vec3> pts;
    for (int v = m.hull_group_start[g]; v < m.hull_group_start[g + 1]; v++)
      if (m.hull_radius[v] == 0.0) pts.push_back(m.hull_xyz[v]);
    for (auto &pl : convex_hull_planes(pts)) plane.insert(plane.end(), pl.begin(), pl.end());
    start.push_back((int)(plane.size() / 4));
  }
}

int render_table(const HostModel &m, std::vector<TrexRenderPrim> &prims, std::vector<float> &planes) {
  std::vector<double> pl;
  std::vector<int> st;
  hull_group_planes(m, pl, st);
  prims.clear();
  planes.clear();
  auto body_of = [&](int v) {
    for (int b = 0; b < m.nb; b++) if (m.hull_start[b] <= v && v < m.hull_start[b + 1]) return b;
    return -1;
  };
  for (size_t g = 0; g + 1 < m.hull_group_start.size(); g++) {
    const int g0 = m.hull_group_start[g], g1 = m.hull_group_start[g + 1];
    int body = -1;
    Vec3 lo{1e300, 1e300, 1e300}, hi{-1e300, -1e300, -1e300};
    for (int v = g0; v < g1; v++) {
      const Vec3 &q = m.hull_xyz[v];
      if (m.hull_radius[v] > 0) {   // primitive collision: a sphere of its own
        TrexRenderPrim s{body_of(v), 0, 0, 1, {(float)q.x, (float)q.y, (float)q.z}, (float)m.hull_radius[v]};
        if (s.body >= 0) prims.push_back(s);
        continue;
      }
      if (body < 0) body = body_of(v);
      lo = {std::min(lo.x, q.x), std::min(lo.y, q.y), std::min(lo.z, q.z)};
      hi = {std::max(hi.x, q.x), std::max(hi.y, q.y), std::max(hi.z, q.z)};
    }
    const int np = st[g + 1] - st[g];
    if (np == 0 || body < 0) continue;
    const Vec3 c{0.5 * (lo.x + hi.x), 0.5 * (lo.y + hi.y), 0.5 * (lo.z + hi.z)};
    double r2 = 0;
    for (int v = g0; v < g1; v++) {
      if (m.hull_radius[v] > 0) continue;
      const Vec3 &q = m.hull_xyz[v];
      r2 = std::max(r2, (q.x - c.x) * (q.x - c.x) + (q.y - c.y) * (q.y - c.y) + (q.z - c.z) * (q.z - c.z));
    }
    // bound rounded up: the kernel skips a hull whose bounding sphere the ray misses
    TrexRenderPrim h{body, (int)(planes.size() / 4), np, 0, {(float)c.x, (float)c.y, (float)c.z},
                     (float)(std::sqrt(r2) * (1 + 1e-5) + 1e-5)};
    prims.push_back(h);
    for (int k = st[g]; k < st[g + 1]; k++)
      for (int j = 0; j < 4; j++) planes.push_back((float)pl[4 * k + j]);
    // padded to a multiple of 8 (the kernel's unrolled step) with copies of the last plane, which change nothing
    const std::vector<float> last(planes.end() - 4, planes.end());
    while ((planes.size() / 4) % 8) planes.insert(planes.end(), last.begin(), last.end());
    prims.back().nplanes = (int)(planes.size() / 4) - prims.back().plane0;
  }
  return (int)prims.size();
}

}  // namespace trex
