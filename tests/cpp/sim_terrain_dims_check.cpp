// Stand-alone host check of simple-mpc_amd/csrc/smpc_sim_terrain_dims.h (the cell-index arithmetic that the terrain kernel calls, the
// sampling and the admission of the simulator's height-field terrain), meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/cpp/sim_terrain_dims_check.cpp -o sim_terrain_dims_check && ./sim_terrain_dims_check
#include "../../simple-mpc_amd/csrc/smpc_sim_terrain_dims.h"
#include <limits>
#include <vector>

using namespace smpc;
#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);                                                      \
      return 1;                                                                                                        \
    }                                                                                                                  \
  } while (0)

static bool has(const std::string & s, const char * w) { return s.find(w) != std::string::npos; }

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- the index arithmetic: 0 <= i <= n - 2 and 0 <= u <= 1 whatever the coordinate; the conversion to int is never undefined ----
  for (int n : {2, 5})
    for (double cell : {0.12, 1.0, 1e-3})
      for (double o : {0.0, -0.7, 3.25})
      {
        std::vector<double> ps = {nan, inf, -inf, 1e300, -1e300, -0.0, 0.0, 1.7976931348623157e308, -1.7976931348623157e308, 5e-324, o, o - 1e-12, o + 1e-12};
        for (int k = 0; k < n; k++) // exact node coordinates and their neighbours, both borders among them
          for (double e : {0.0, -1e-13, 1e-13})
            ps.push_back(o + k * cell + e);
        ps.push_back(o + (n - 1) * cell + 10.0);
        ps.push_back(o - 10.0);
        for (double p : ps)
        {
          const SimTerrainCell c = sim_terrain_cell(p, o, cell, n);
          CHECK(c.i >= 0 && c.i <= n - 2);
          CHECK(c.u >= 0.0 && c.u <= 1.0);
          if (!(std::fabs((p - o) / cell) <= 1.7976931348623157e308)) // NaN and +-inf: index 0, fraction 0
            CHECK(c.i == 0 && c.u == 0.0);
        }
        // a NaN or infinite origin or cell is no different
        for (double bad : {nan, inf, -inf})
        {
          const SimTerrainCell a = sim_terrain_cell(0.3, bad, cell, n), b = sim_terrain_cell(0.3, o, bad, n);
          CHECK(a.i == 0 && a.u == 0.0 && b.i >= 0 && b.i <= n - 2 && b.u >= 0.0 && b.u <= 1.0);
        }
        // inside: the cell and the fraction
        const SimTerrainCell first = sim_terrain_cell(o, o, cell, n), last = sim_terrain_cell(o + (n - 1) * cell + 1.0, o, cell, n);
        CHECK(first.i == 0 && first.u == 0.0 && last.i == n - 2 && last.u == 1.0);
        const SimTerrainCell below = sim_terrain_cell(o - 1.0, o, cell, n), zero = sim_terrain_cell(-0.0, 0.0, cell, n);
        CHECK(below.i == 0 && below.u == 0.0 && zero.i == 0 && zero.u == 0.0 && !std::signbit(zero.u));
      }
  {
    const SimTerrainCell c = sim_terrain_cell(0.3 + 2.25 * 0.5, 0.3, 0.5, 5);
    CHECK(c.i == 2 && std::fabs(c.u - 0.25) < 1e-12);
    const SimTerrainCell d = sim_terrain_cell(0.3 + 4.0 * 0.5, 0.3, 0.5, 5); // the last node belongs to the last cell
    CHECK(d.i == 3 && std::fabs(d.u - 1.0) < 1e-12);
  }
  // ---- the sampling: a flat patch is the plane exactly; a tilted one has the plane's normal ----
  {
    const SimTerrainSample f = sim_terrain_sample(0.37, 0.37, 0.37, 0.37, 0.3, 0.9, 0.12);
    CHECK(f.h == 0.37 && f.n[0] == 0.0 && f.n[1] == 0.0 && f.n[2] == 1.0 && !std::signbit(f.n[0]) && !std::signbit(f.n[1]));
    const SimTerrainSample t = sim_terrain_sample(0.0, 0.1, -0.2, -0.1, 0.5, 0.5, 1.0); // h = 0.1 x - 0.2 y
    const double s = 1.0 / std::sqrt(1.05);
    CHECK(std::fabs(t.h - (-0.05)) < 1e-15 && std::fabs(t.n[0] + 0.1 * s) < 1e-15 && std::fabs(t.n[1] - 0.2 * s) < 1e-15 && std::fabs(t.n[2] - s) < 1e-15);
  }
  // ---- sizes ----
  CHECK(sim_terrain_height_bytes(3, 4, 5) == 480 && sim_terrain_tile_bytes(7) == 28 && sim_terrain_origin_bytes(7) == 112);
  CHECK(sim_terrain_normal_bytes(2, 8) == 384 && sim_terrain_hlast_bytes(2, 8) == 128);
  // ---- admission: heap arrays of exactly the admitted sizes, so that a read past them is the sanitizer's to report ----
  const int B = 3, T = 2, ny = 4, nx = 6;
  std::vector<double> good((size_t)T * ny * nx);
  for (size_t k = 0; k < good.size(); k++)
    good[k] = 0.3 + 0.01 * (double)((k * 7) % 5);
  std::vector<int32_t> tile = {0, 1, 1};
  std::vector<double> origin = {0.0, 0.0, 0.5, -0.5, -1.0, 2.0};
  auto make = [&](const std::vector<double> & h) {
    smpc_terrain_settings t;
    t.nx = nx;
    t.ny = ny;
    t.tiles = T;
    t.cell = 0.12;
    t.heights = h.data();
    t.tile = tile.data();
    t.origin = origin.data();
    return t;
  };
  {
    smpc_terrain_settings t = make(good);
    CHECK(sim_terrain_admission_error(B, nullptr).empty());
    CHECK(sim_terrain_admission_error(B, &t).empty());
    t.tile = nullptr;
    t.origin = nullptr;
    CHECK(sim_terrain_admission_error(B, &t).empty());
    std::vector<double> two = {0.1, 0.1, 0.1, 0.1};
    smpc_terrain_settings s = make(two);
    s.nx = s.ny = 2;
    s.tiles = 1;
    s.tile = nullptr;
    CHECK(sim_terrain_admission_error(B, &s).empty());
    // the steepest admitted corner: hx^2 + hy^2 = 3 exactly is accepted, a little more is not
    std::vector<double> edge = {0.0, 1.0, 1.0, 2.0}; // cell 1: hx = 1, hy = 1 at every corner
    smpc_terrain_settings e = make(edge);
    e.nx = e.ny = 2;
    e.tiles = 1;
    e.tile = nullptr;
    e.cell = 1.0;
    CHECK(sim_terrain_admission_error(B, &e).empty());
    e.cell = 0.8; // 1.5625 + 1.5625 > 3
    CHECK(has(sim_terrain_admission_error(B, &e), "slope[0][0][0]"));
  }
  // refused: every refusal the header names, with the field and the first offending index
  {
    smpc_terrain_settings t = make(good);
    t.nx = 1;
    CHECK(has(sim_terrain_admission_error(B, &t), "terrain: nx = 1"));
    t = make(good);
    t.ny = 0;
    CHECK(has(sim_terrain_admission_error(B, &t), "ny = 0"));
    t = make(good);
    t.tiles = 0;
    CHECK(has(sim_terrain_admission_error(B, &t), "tiles = 0"));
    t = make(good);
    t.tiles = 4096;
    t.nx = t.ny = 2048; // (refused before a height is read)
    CHECK(has(sim_terrain_admission_error(B, &t), "cap"));
    t.tiles = 1;
    t.nx = 2049;
    CHECK(has(sim_terrain_admission_error(B, &t), "cap"));
    for (double c : {0.0, -0.1, nan, inf, -inf})
    {
      t = make(good);
      t.cell = c;
      CHECK(has(sim_terrain_admission_error(B, &t), "cell"));
    }
    t = make(good);
    t.heights = nullptr;
    CHECK(has(sim_terrain_admission_error(B, &t), "heights is null"));
    for (double v : {nan, inf, -inf})
    {
      std::vector<double> h = good;
      h[(size_t)(1 * ny + 2) * nx + 3] = v;
      h.back() = nan;
      t = make(h);
      CHECK(has(sim_terrain_admission_error(B, &t), "heights[1][2][3]"));
    }
    t = make(good);
    tile = {0, 2, -1};
    CHECK(has(sim_terrain_admission_error(B, &t), "tile[1] = 2"));
    CHECK(sim_terrain_admission_error(1, &t).empty()); // (robot 0 alone is fine)
    tile = {0, 1, -1};
    CHECK(has(sim_terrain_admission_error(B, &t), "tile[2] = -1"));
    tile = {0, 1, 1};
    origin[3] = nan;
    origin[4] = inf;
    CHECK(has(sim_terrain_admission_error(B, &t), "origin[1][1]"));
    origin[3] = 0.0;
    CHECK(has(sim_terrain_admission_error(B, &t), "origin[2][0]"));
    origin[4] = 0.0;
    CHECK(sim_terrain_admission_error(B, &t).empty());
    std::vector<double> h = good;
    h[(size_t)(1 * ny + 2) * nx + 3] += 0.3; // the node is a corner of four cells; the first of them in [tile][j][i] order is named
    t = make(h);
    CHECK(has(sim_terrain_admission_error(B, &t), "slope[1][1][2]"));
  }
  std::printf("sim_terrain_dims_check: ok\n");
  return 0;
}
