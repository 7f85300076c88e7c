// Off-road flags straight from a device-resident drivable-area map (get_off_road_matrix, traj_evaluator.py:273-331, without the raster):
// the town's drivable polygons stay in HBM (drivable_grid.h), and a rollout point is decided against the few polygons near it.
//
// THE RULE.  Pixel (px, py) of a CBV's (H, W) raster is drivable iff, for some polygon of the map, the pixel centre lies inside or on the
// boundary of the polygon with the vertices v_i = int32(rint(global_to_pixel(vertex_i))): global_to_pixel is the reference's (:324-327) in
// fp64 without fused multiply-add -- d = p - origin, (d.x c + d.y s, -d.x s + d.y c) / (res, -res) + (H / 2, W / 2), res rounded to fp32 first
// and the HEIGHT going to x (the quirk rift_group_advantage_tick_ex reproduces).  Interior: even-odd, half-open in y; boundary: inclusive.
// The arithmetic on the rounded vertices is exact (fp64 on integers below 2^26).  A zero-length edge (a ring closed by repeating its first
// vertex) counts nothing and lies on a vertex; a polygon that collapses to a line after rounding clears the pixels of that line.
// This is NOT cv2.fillPoly bit for bit: a scanline rasteriser also sets the 8-connected outline it draws along every edge, whose pixels lie
// up to half a pixel outside the mathematical polygon ("Unpinned").  Hence opt-in.
#pragma once
#include "adv.h"
#include "drivable_grid.h"

namespace rift {

struct DrivableMapDev {                          // the images of RiftCtxCore::dmap as a kernel takes them
  const double* vertices; const double* aabb;
  const int* poly_start; const int* cell_start; const int* cell_poly;
  double x0, y0, cell, margin;
  int nx, ny;
};

struct RasterPose { double ox, oy, c, s, res, off_x, off_y, inv_res; };      // origin, cos / sin of the heading, metres per pixel, (H / 2, W / 2) as fp32; inv_res: drivable_inv_res

// 1 / res where that is exact (res a power of two, as 0.5 and 0.25: x / res and x * (1 / res) are then the same bits), else 0: divide
inline double drivable_inv_res(double res) {
  int e;
  return std::frexp(res, &e) == 0.5 ? 1.0 / res : 0.0;
}

// vertex -> its rounded pixel: the arithmetic of off_road_body (adv.h), on an fp64 point.  The pixel stays in fp64: an integer below 2^26 in
// magnitude for every polygon near enough to be tested, so that the products and the difference of the edge tests below are exact.
__device__ __forceinline__ void drivable_vertex_pixel(const RasterPose& q, double x, double y, double& vx, double& vy) {
  const double dx = x - q.ox, dy = y - q.oy;
  const double lx = __dadd_rn(__dmul_rn(dx, q.c), __dmul_rn(dy, q.s));
  const double ly = __dadd_rn(__dmul_rn(dx, -q.s), __dmul_rn(dy, q.c));
  if (q.inv_res != 0.0) {                        // (wave-uniform; the product with a power of two is exact: the same bits as the quotient)
    vx = rint(__dadd_rn(__dmul_rn(lx, q.inv_res), q.off_x));
    vy = rint(__dadd_rn(__dmul_rn(ly, -q.inv_res), q.off_y));
  } else {
    vx = rint(lx / q.res + q.off_x);
    vy = rint(ly / -q.res + q.off_y);
  }
}

__device__ __forceinline__ bool pixel_drivable(const DrivableMapDev& m, const RasterPose& q, int px, int py) {
  // the pixel centre back in the world: for culling only (the margin of the cell lists and of the box test covers its rounding)
  const double lx = ((double)px - q.off_x) * q.res, ly = ((double)py - q.off_y) * -q.res;
  const double wx = q.ox + (lx * q.c - ly * q.s), wy = q.oy + (lx * q.s + ly * q.c);
  const int ix = drivable_cell_of(wx, m.x0, m.cell, m.nx), iy = drivable_cell_of(wy, m.y0, m.cell, m.ny);
  if (ix < 0 || iy < 0) return false;            // outside the grid: outside every inflated box
  const int c0 = m.cell_start[iy * m.nx + ix], c1 = m.cell_start[iy * m.nx + ix + 1];
  const double X = px, Y = py;
  for (int e = c0; e < c1; ++e) {
    const int k = m.cell_poly[e];
    const double* b = m.aabb + (size_t)k * 4;
    if (wx < b[0] - m.margin || wx > b[2] + m.margin || wy < b[1] - m.margin || wy > b[3] + m.margin) continue;
    const int v0 = m.poly_start[k], v1 = m.poly_start[k + 1];
    double ax, ay;
    drivable_vertex_pixel(q, m.vertices[2 * (size_t)(v1 - 1)], m.vertices[2 * (size_t)(v1 - 1) + 1], ax, ay);      // the closing edge first: last -> first
    bool inside = false, on_edge = false;
    for (int i = v0; i < v1; ++i) {
      double bx, by;
      drivable_vertex_pixel(q, m.vertices[2 * (size_t)i], m.vertices[2 * (size_t)i + 1], bx, by);
      const double ex = bx - ax, ey = by - ay;
      const double cross = __dadd_rn(__dmul_rn(ex, Y - ay), -__dmul_rn(ey, X - ax));      // integers: exact
      if (cross == 0.0 && X >= fmin(ax, bx) && X <= fmax(ax, bx) && Y >= fmin(ay, by) && Y <= fmax(ay, by)) on_edge = true;
      // even-odd, half-open in y: the edge crosses the row of the centre and does so to its right.  x of the crossing > X
      //   <=>  (X - ax) * ey < (Y - ay) * ex for ey > 0 (reversed for ey < 0)   <=>   cross > 0 for ey > 0, cross < 0 for ey < 0
      if ((ay > Y) != (by > Y)) { if (ey > 0.0 ? cross > 0.0 : cross < 0.0) inside = !inside; }
      ax = bx; ay = by;
    }
    if (inside || on_edge) return true;
  }
  return false;
}

// the map's decision on the pixel of a rollout point (off_road_pixel, adv.h): off road = inside the raster and not drivable
__device__ __forceinline__ uint8_t off_road_map_flag(double px, double py, const DrivableMapDev& m, const RasterPose& q, int H, int W) {
  uint8_t off = 0;
  if (px >= 0.0 && px < (double)W && py >= 0.0 && py < (double)H) off = pixel_drivable(m, q, (int)px, (int)py) ? 0 : 1;
  return off;
}

// one thread per rollout point: the pixel is off_road_body's, bit for bit
__device__ __forceinline__ void off_road_map_body(const float* __restrict__ pts /*(n,2)*/, int n, const DrivableMapDev& m, const RasterPose& q, int H, int W,
                                                  uint8_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double px, py;
  off_road_pixel((double)pts[2 * i], (double)pts[2 * i + 1], q.ox, q.oy, q.c, q.s, q.res, -q.res, q.off_x, q.off_y, px, py);
  out[i] = off_road_map_flag(px, py, m, q, H, W);
}
__global__ __launch_bounds__(256) void off_road_map_kernel(const float* __restrict__ pts, int n, const DrivableMapDev m, const RasterPose q, int H, int W,
                                                           uint8_t* __restrict__ out) {
  off_road_map_body(pts, n, m, q, H, W, out);
}

// one thread per pixel of the (H, W) mask the reference would hand to the lookup: 1 = off road, 0 = drivable
__global__ __launch_bounds__(256) void drivable_raster_kernel(const DrivableMapDev m, const RasterPose q, int H, int W, uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int py = i / W, px = i - py * W;
  mask[i] = pixel_drivable(m, q, px, py) ? 0 : 1;
}

}  // namespace rift
