"""csrc/drivable_grid.h on the CPU: the grid of the drivable-area map and its owning device images, in the pattern of tests/test_devmem_host.py.

The header is host-only, so a stand-alone program (its own main, built by g++ with the address and undefined-behaviour sanitizers, run
directly) builds the grid of a map it reads from a file and prints it; the cell lists are compared here with the numpy restatement
(tests/drivable_cases.py: grid_lists).  The program itself checks the CSR offsets, every refusal and its message, the resolution rule and
the all-or-nothing allocation of the images against counting fakes of the two allocation hooks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import drivable_cases as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>
#include "drivable_grid.h"

static std::set<void*> live;
static long allocs = 0, frees = 0, fail_in = 0;      // fail_in = n: the n-th allocation from now fails
int rift_dev_alloc(void** p, size_t bytes) {
  if (fail_in > 0 && --fail_in == 0) return 2;
  void* q = malloc(bytes ? bytes : 1);
  live.insert(q); ++allocs; *p = q;
  return 0;
}
void rift_dev_free(void* p) {
  if (!live.erase(p)) { fprintf(stderr, "free of an address that is not live\n"); abort(); }
  free(p); ++frees;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static bool refused(const char* got, const char* part) {
  if (!got || !strstr(got, part)) { fprintf(stderr, "expected a refusal with \"%s\", got \"%s\"\n", part, got ? got : "(accepted)"); return false; }
  return true;
}

int main(int argc, char** argv) {
  CHECK(argc == 4);
  const double cell = atof(argv[2]), margin = atof(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int np = 0;
  CHECK(fread(&np, 4, 1, f) == 1);
  std::vector<int32_t> start((size_t)np + 1);
  CHECK(fread(start.data(), 4, start.size(), f) == start.size());
  std::vector<double> v((size_t)start[np] * 2);
  CHECK(fread(v.data(), 8, v.size(), f) == v.size());
  fclose(f);

  DrivableGrid g;
  const char* why = drivable_grid_build(v.data(), start.data(), np, cell, margin, &g);
  CHECK(why == nullptr);
  // the CSR offsets: start at 0, never decrease, end at the number of entries; the longest list is what max_list says
  CHECK(g.n_polys == np && g.n_vertices == start[np] && g.cell == cell && g.margin == margin);
  CHECK(g.cell_start.size() == (size_t)g.nx * g.ny + 1 && g.cell_start[0] == 0 && (size_t)g.cell_start.back() == g.cell_poly.size());
  int longest = 0;
  for (size_t c = 0; c + 1 < g.cell_start.size(); ++c) {
    CHECK(g.cell_start[c + 1] >= g.cell_start[c]);
    longest = std::max(longest, g.cell_start[c + 1] - g.cell_start[c]);
    for (int e = g.cell_start[c]; e < g.cell_start[c + 1]; ++e) {
      CHECK(g.cell_poly[e] >= 0 && g.cell_poly[e] < np);
      if (e > g.cell_start[c]) CHECK(g.cell_poly[e] > g.cell_poly[e - 1]);      // map order, no polygon twice
    }
  }
  CHECK(longest == g.max_list);
  // the cell of a coordinate: the grid's own statement of it, at its borders
  CHECK(drivable_cell_of(g.x0, g.x0, cell, g.nx) == 0 && drivable_cell_of(g.x0 - 1e-9, g.x0, cell, g.nx) == -1);
  CHECK(drivable_cell_of(g.x0 + cell * g.nx, g.x0, cell, g.nx) == -1 && drivable_cell_of(g.x0 + cell * g.nx - 1e-6, g.x0, cell, g.nx) == g.nx - 1);
  printf("grid %.17g %.17g %d %d %d\n", g.x0, g.y0, g.nx, g.ny, g.max_list);
  for (int k = 0; k < np; ++k) printf("box %d %.17g %.17g %.17g %.17g\n", k, g.aabb[4 * k], g.aabb[4 * k + 1], g.aabb[4 * k + 2], g.aabb[4 * k + 3]);
  for (int iy = 0; iy < g.ny; ++iy) for (int ix = 0; ix < g.nx; ++ix) {
    const size_t c = (size_t)iy * g.nx + ix;
    if (g.cell_start[c + 1] == g.cell_start[c]) continue;
    printf("cell %d %d", ix, iy);
    for (int e = g.cell_start[c]; e < g.cell_start[c + 1]; ++e) printf(" %d", g.cell_poly[e]);
    printf("\n");
  }

  // ---- refusals, each with its message; a refused build leaves the output alone
  const double tri[6] = {0, 0, 4, 0, 0, 4};
  const int32_t s3[2] = {0, 3}, s2[2] = {0, 2}, bad0[2] = {1, 4}, down[3] = {0, 3, 2};
  DrivableGrid keep; keep.nx = 77;
  CHECK(refused(drivable_grid_build(tri, s2, 1, 16, 1, &keep), "fewer than 3 vertices") && keep.nx == 77);
  CHECK(refused(drivable_grid_build(tri, down, 2, 16, 1, &keep), "not monotone"));
  CHECK(refused(drivable_grid_build(tri, bad0, 1, 16, 1, &keep), "poly_start[0]"));
  CHECK(refused(drivable_grid_build(tri, s3, 1, 0.0, 1, &keep), "cell <= 0"));
  CHECK(refused(drivable_grid_build(tri, s3, 1, -2.0, 1, &keep), "cell <= 0"));
  CHECK(refused(drivable_grid_build(tri, s3, 1, std::numeric_limits<double>::quiet_NaN(), 1, &keep), "cell <= 0"));
  CHECK(refused(drivable_grid_build(tri, s3, 1, 16, -0.5, &keep), "margin < 0"));
  CHECK(refused(drivable_grid_build(tri, s3, -1, 16, 1, &keep), "n_polys < 0"));
  CHECK(refused(drivable_grid_build(nullptr, s3, 1, 16, 1, &keep), "null"));
  double nan_tri[6] = {0, 0, 4, std::numeric_limits<double>::quiet_NaN(), 0, 4}, inf_tri[6] = {0, 0, std::numeric_limits<double>::infinity(), 0, 0, 4};
  CHECK(refused(drivable_grid_build(nan_tri, s3, 1, 16, 1, &keep), "not finite"));
  CHECK(refused(drivable_grid_build(inf_tri, s3, 1, 16, 1, &keep), "not finite"));
  const double wide[6] = {0, 0, 1e9, 0, 0, 1e9};
  CHECK(refused(drivable_grid_build(wide, s3, 1, 1.0, 1, &keep), "2^24 cells") && keep.nx == 77);
  // accepted at the edges: margin 0, one triangle, and no polygons at all (an empty grid: every point is outside it)
  DrivableGrid one, none;
  CHECK(drivable_grid_build(tri, s3, 1, 16, 0.0, &one) == nullptr && one.nx == 1 && one.ny == 1 && one.max_list == 1 && one.cell_poly.size() == 1);
  CHECK(drivable_grid_build(nullptr, nullptr, 0, 16, 1, &none) == nullptr && none.nx == 0 && none.ny == 0 && none.cell_start.size() == 1 && none.cell_poly.empty());
  CHECK(drivable_cell_of(0.0, none.x0, none.cell, none.nx) == -1);
  // ---- the resolution a map can decide: res * sqrt(2) <= margin (res as the caller rounds it)
  CHECK(drivable_res_refusal(1.0, 0.5) == nullptr && drivable_res_refusal(1.0, 0.25) == nullptr && drivable_res_refusal(1.0, 0.7071) == nullptr);
  CHECK(refused(drivable_res_refusal(1.0, 1.0), "margin") && refused(drivable_res_refusal(1.0, 0.7072), "margin") && refused(drivable_res_refusal(0.0, 0.5), "margin"));
  CHECK(refused(drivable_res_refusal(1.0, 0.0), "resolution <= 0") && refused(drivable_res_refusal(1.0, std::numeric_limits<double>::quiet_NaN()), "resolution <= 0"));
  // ---- the images: all five or none
  {
    DrivableImages im;
    CHECK(im.reserve(g) == 0 && live.size() == 5);
    CHECK(im.bytes() == (g.n_vertices * 2 + g.aabb.size()) * 8 + ((size_t)np + 1 + g.cell_start.size() + g.cell_poly.size()) * 4);
    for (size_t i = 0; i < g.cell_poly.size(); ++i) im.cell_poly.get()[i] = g.cell_poly[i];      // (the sanitizer checks the size)
    for (size_t i = 0; i < g.aabb.size(); ++i) im.aabb.get()[i] = g.aabb[i];
    im.reset();
    CHECK(live.empty() && im.bytes() == 0);
    for (int n = 1; n <= 5; ++n) {                  // the n-th allocation fails: nothing stays
      fail_in = n;
      CHECK(im.reserve(g) != 0 && live.empty() && im.vertices.get() == nullptr && im.cell_poly.get() == nullptr);
    }
    CHECK(im.reserve(g) == 0 && live.size() == 5);
    CHECK(im.reserve(none) == 0 && live.size() == 5);      // a smaller map fits where a larger one was
  }                                                        // destructor of full images
  CHECK(live.empty() && allocs == frees && allocs > 0);
  printf("ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("drivable_host")
    src = d / "drivable_host.cpp"
    src.write_text(PROGRAM)
    out = d / "drivable_host"
    subprocess.check_call([gxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(REPO, "rift_amd", "csrc"), str(src), "-o", str(out)])
    return str(out)


def run(exe, tmp_path, polys, cell, margin):
    start = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    path = tmp_path / "map.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(polys)).tobytes() + start.tobytes() + np.concatenate(polys, 0).astype(np.float64).tobytes())
    r = subprocess.run([exe, str(path), repr(float(cell)), repr(float(margin))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[-2] == "ok"
    head = lines[0].split()
    grid = {"x0": float(head[1]), "y0": float(head[2]), "nx": int(head[3]), "ny": int(head[4]), "max_list": int(head[5]), "lists": {}, "boxes": []}
    for ln in lines[1:]:
        w = ln.split()
        if w and w[0] == "cell":
            grid["lists"][(int(w[1]), int(w[2]))] = [int(x) for x in w[3:]]
        elif w and w[0] == "box":
            grid["boxes"].append([float(x) for x in w[2:]])
    return grid


@pytest.mark.parametrize("name,polys,cell,margin", [
    ("gpu_map", D.gpu_map(), D.GPU_CELL, D.GPU_MARGIN),
    ("town", D.lane_map(3, 300, span=900.0, centre=(250.0, -4000.0)), 16.0, 1.0),
    ("small_cells", D.lane_map(4, 40, span=120.0), 5.0, 2.5),
    ("no_margin", D.lane_map(6, 25, span=80.0), 32.0, 0.0),
], ids=lambda v: v if isinstance(v, str) else "")
def test_every_polygon_is_in_exactly_the_cells_its_inflated_box_touches(exe, tmp_path, name, polys, cell, margin):
    got = run(exe, tmp_path, polys, cell, margin)
    want = D.grid_lists(polys, cell, margin)
    assert (got["x0"], got["y0"], got["nx"], got["ny"]) == (want["x0"], want["y0"], want["nx"], want["ny"])
    assert np.array_equal(np.asarray(got["boxes"]), want["boxes"])
    assert got["lists"] == want["lists"]
    assert got["max_list"] == max(len(v) for v in want["lists"].values())
    # and stated once more without the restatement's arithmetic: a polygon is listed in a cell iff the closed cell square meets its
    # inflated box (the half-open cell and the box's closed end differ only on a cell border, which these seeded maps do not hit)
    for (ix, iy), members in list(got["lists"].items())[::7]:
        cx0, cy0 = got["x0"] + ix * cell, got["y0"] + iy * cell
        for k, b in enumerate(want["boxes"]):
            meets = b[0] - margin < cx0 + cell and b[2] + margin >= cx0 and b[1] - margin < cy0 + cell and b[3] + margin >= cy0
            assert meets == (k in members), (ix, iy, k)


def test_the_gpu_map_shows_what_its_docstring_says():
    """The facts tests/test_gpu_drivable_map.py relies on, on the restated grid: the five-cell strip, the cell that lists the square through
    the margin only, empty cells, and the sizes of the hand-made polygons."""
    polys = D.gpu_map()
    g = D.grid_lists(polys, D.GPU_CELL, D.GPU_MARGIN)
    assert len(polys) == 40 and len(polys[36]) == 3 and len(polys[37]) == 200
    cells38 = [c for c, l in g["lists"].items() if 38 in l]
    assert len({c[0] for c in cells38}) == 5 and len({c[1] for c in cells38}) == 1
    cells39 = sorted(c for c, l in g["lists"].items() if 39 in l)
    bare = D.grid_lists(polys, D.GPU_CELL, 0.0)                  # without a margin the square sits in one cell (the grid's corner moves by the margin: compare counts)
    assert len(cells39) == 2 and len([c for c, l in bare["lists"].items() if 39 in l]) == 1
    x_border = g["x0"] + cells39[1][0] * D.GPU_CELL
    assert g["boxes"][39][2] < x_border <= g["boxes"][39][2] + D.GPU_MARGIN      # the box ends short of the border, the inflated box crosses it
    assert any((i, j) not in g["lists"] for i in range(g["nx"]) for j in range(g["ny"]))
