// The drivable-area map of a town on the host side (host-only: no HIP header, compiles with a plain C++17 compiler): the polygons'
// world bounding boxes and a uniform grid over them in CSR form, and the owning device images of the five arrays a kernel reads
// (drivable_map.h).  The grid is a CULLING structure only -- which polygons a point has to be tested against; the test itself is the
// device's.  A polygon is listed in every cell its bounding box, inflated by `margin`, touches.  Why that is enough: a raster pixel is
// drivable when its centre lies in or on the polygon of the ROUNDED pixel vertices; rounding moves a vertex by at most half a pixel per
// axis, so such a centre is within res * sqrt(2) / 2 metres of the world polygon, hence of its bounding box.  A call is refused unless
// res * sqrt(2) <= margin (drivable_res_refusal): twice that distance, the rest is room for the rounding of the fp64 arithmetic.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "devmem.h"

#define RIFT_DRIVABLE_MAX_CELLS (1 << 24)

struct DrivableGrid {
  std::vector<double> aabb;                      // (n_polys, 4): min x, min y, max x, max y of the world vertices (not inflated)
  std::vector<int32_t> cell_start, cell_poly;    // CSR: the polygons of cell (ix, iy) are cell_poly[cell_start[iy * nx + ix] .. cell_start[iy * nx + ix + 1])
  double x0 = 0.0, y0 = 0.0, cell = 0.0, margin = 0.0;      // cell (ix, iy) = [x0 + ix * cell, x0 + (ix + 1) * cell) x [y0 + iy * cell, ...)
  int nx = 0, ny = 0, n_polys = 0, n_vertices = 0, max_list = 0;
};

// The cell index of a coordinate along one axis, or -1 outside the grid.  The one statement of it: the builder and the kernel call this.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int drivable_cell_of(double v, double v0, double cell, int n) {
  const double f = floor((v - v0) / cell);
  return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

// nullptr, or why the map is refused.  vertices: (poly_start[n_polys], 2) f64 in the global frame; polygon k owns the vertices
// poly_start[k] .. poly_start[k + 1] (a ring may repeat its first vertex as its last).  No polygons at all is a valid map: an empty grid.
inline const char* drivable_grid_build(const double* vertices, const int32_t* poly_start, int n_polys, double cell, double margin, DrivableGrid* out) {
  if (!out) return "no output";
  if (n_polys < 0) return "n_polys < 0";
  if (!(cell > 0.0) || !std::isfinite(cell)) return "cell <= 0 or not finite";
  if (!(margin >= 0.0) || !std::isfinite(margin)) return "margin < 0 or not finite";
  if (n_polys > 0 && (!vertices || !poly_start)) return "null vertices or poly_start";
  DrivableGrid g;
  g.cell = cell; g.margin = margin; g.n_polys = n_polys;
  if (n_polys == 0) { g.cell_start.assign(1, 0); *out = std::move(g); return nullptr; }
  if (poly_start[0] != 0) return "poly_start[0] != 0";
  for (int k = 0; k < n_polys; ++k) {
    if (poly_start[k + 1] < poly_start[k]) return "poly_start is not monotone";
    if (poly_start[k + 1] - poly_start[k] < 3) return "a polygon with fewer than 3 vertices";
  }
  g.n_vertices = poly_start[n_polys];
  for (int i = 0; i < 2 * g.n_vertices; ++i) if (!std::isfinite(vertices[i])) return "a vertex coordinate that is not finite";
  g.aabb.resize((size_t)n_polys * 4);
  double lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  for (int k = 0; k < n_polys; ++k) {
    double a = INFINITY, b = INFINITY, c = -INFINITY, d = -INFINITY;
    for (int i = poly_start[k]; i < poly_start[k + 1]; ++i) {
      a = std::fmin(a, vertices[2 * i]); b = std::fmin(b, vertices[2 * i + 1]); c = std::fmax(c, vertices[2 * i]); d = std::fmax(d, vertices[2 * i + 1]);
    }
    double* q = &g.aabb[(size_t)k * 4];
    q[0] = a; q[1] = b; q[2] = c; q[3] = d;
    lo_x = std::fmin(lo_x, a); lo_y = std::fmin(lo_y, b); hi_x = std::fmax(hi_x, c); hi_y = std::fmax(hi_y, d);
  }
  g.x0 = lo_x - margin; g.y0 = lo_y - margin;
  const double fx = std::floor((hi_x + margin - g.x0) / cell) + 1.0, fy = std::floor((hi_y + margin - g.y0) / cell) + 1.0;
  if (!(fx * fy <= (double)RIFT_DRIVABLE_MAX_CELLS)) return "the grid would have more than 2^24 cells: use a larger cell";
  g.nx = (int)fx; g.ny = (int)fy;
  // the cells an inflated box touches: both ends through drivable_cell_of (inside by construction of x0 / nx)
  auto span = [&](int k, int& ix0, int& ix1, int& iy0, int& iy1) {
    const double* q = &g.aabb[(size_t)k * 4];
    ix0 = drivable_cell_of(q[0] - margin, g.x0, cell, g.nx); ix1 = drivable_cell_of(q[2] + margin, g.x0, cell, g.nx);
    iy0 = drivable_cell_of(q[1] - margin, g.y0, cell, g.ny); iy1 = drivable_cell_of(q[3] + margin, g.y0, cell, g.ny);
    if (ix0 < 0) ix0 = 0;
    if (iy0 < 0) iy0 = 0;
    if (ix1 < 0) ix1 = g.nx - 1;
    if (iy1 < 0) iy1 = g.ny - 1;
  };
  std::vector<int32_t> count((size_t)g.nx * g.ny + 1, 0);
  for (int k = 0; k < n_polys; ++k) {
    int ix0, ix1, iy0, iy1; span(k, ix0, ix1, iy0, iy1);
    for (int iy = iy0; iy <= iy1; ++iy) for (int ix = ix0; ix <= ix1; ++ix) ++count[(size_t)iy * g.nx + ix + 1];
  }
  long long total = 0;
  for (size_t i = 1; i < count.size(); ++i) {
    g.max_list = count[i] > g.max_list ? count[i] : g.max_list;
    total += count[i];
    if (total > 0x7fffffffLL) return "more than 2^31 cell entries: use a larger cell";
    count[i] = (int32_t)total;
  }
  g.cell_start = count;
  g.cell_poly.resize((size_t)total);
  std::vector<int32_t> fill(g.cell_start.begin(), g.cell_start.end() - 1);
  for (int k = 0; k < n_polys; ++k) {            // polygon order inside a cell = map order
    int ix0, ix1, iy0, iy1; span(k, ix0, ix1, iy0, iy1);
    for (int iy = iy0; iy <= iy1; ++iy) for (int ix = ix0; ix <= ix1; ++ix) g.cell_poly[(size_t)fill[(size_t)iy * g.nx + ix]++] = k;
  }
  *out = std::move(g);
  return nullptr;
}

// nullptr, or why a raster of resolution `res` (metres per pixel) cannot be decided from a map built with `margin`
inline const char* drivable_res_refusal(double margin, double res) {
  if (!(res > 0.0) || !std::isfinite(res)) return "resolution <= 0 or not finite";
  if (res * std::sqrt(2.0) > margin) return "resolution * sqrt(2) > the map's margin: load the map with a larger margin";
  return nullptr;
}

// The device images of one map.  reserve(): room for the grid `g`; on failure everything is released (a map is used whole or not at all).
struct DrivableImages {
  DevBuf<double> vertices, aabb;
  DevBuf<int32_t> poly_start, cell_start, cell_poly;
  int reserve(const DrivableGrid& g) {
    int rc = vertices.reserve((size_t)g.n_vertices * 2);
    if (!rc) rc = aabb.reserve(g.aabb.size());
    if (!rc) rc = poly_start.reserve((size_t)g.n_polys + 1);
    if (!rc) rc = cell_start.reserve(g.cell_start.size());
    if (!rc) rc = cell_poly.reserve(g.cell_poly.size());
    if (rc) reset();
    return rc;
  }
  void reset() { vertices.reset(); aabb.reset(); poly_start.reset(); cell_start.reset(); cell_poly.reset(); }
  size_t bytes() const { return (vertices.cap() + aabb.cap()) * sizeof(double) + (poly_start.cap() + cell_start.cap() + cell_poly.cap()) * sizeof(int32_t); }
};
