// smpc_sim_terrain_dims.h -- host-side admission, sizes and the cell-index arithmetic of the simulator's per-robot height-field terrain
// (smpc_sim_ground_joint_rt.h: sim_ground_terrain_rt_body): which smpc_terrain_settings a handle accepts, the sizes of the
// arrays, and sim_terrain_cell / sim_terrain_sample, the ONE implementation of the sampling that the kernel, the host and the stand-alone
// program tests/cpp/sim_terrain_dims_check.cpp all call.  Plain C++ with no backend behind it; under a backend the two sampling
// functions are host-and-device functions.
#pragma once
#include "smpc_sim_ground_dims.h"
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>

#ifdef SMPC_HD
#define SMPC_TERRAIN_FN SMPC_HD
#else
#define SMPC_TERRAIN_FN inline
#endif

namespace smpc
{
  // the cap on tiles ny nx: 4 194 304 nodes (32 MiB of doubles), so that every node index fits an int with room to spare
  constexpr long long SIM_TERRAIN_MAX_NODES = 1ll << 22;
  constexpr double SIM_TERRAIN_MAX_SLOPE2 = 3.0; // hx^2 + hy^2 <= 3 at every cell corner: n.z >= 0.5 (the rule of DESIGN 3.24)

  inline size_t sim_terrain_height_bytes(int tiles, int ny, int nx) { return (size_t)tiles * (size_t)ny * (size_t)nx * sizeof(double); }
  inline size_t sim_terrain_tile_bytes(int n) { return (size_t)n * sizeof(int); }
  inline size_t sim_terrain_origin_bytes(int n) { return (size_t)n * 2 * sizeof(double); }
  inline size_t sim_terrain_normal_bytes(int n, int npts) { return (size_t)n * (size_t)npts * 3 * sizeof(double); }
  inline size_t sim_terrain_hlast_bytes(int n, int npts) { return (size_t)n * (size_t)npts * sizeof(double); }

  // cell index i in [0, n - 2] and fraction u in [0, 1] of coordinate p along an axis of n >= 2 nodes, spacing `cell`, node 0 at o:
  // x = (p - o) / cell clamped to [0, n - 1] IN DOUBLE, before any conversion to an integer; i = min(floor(x), n - 2); u = x - i.  The
  // selects are written so that a NaN (every comparison false) or a +-inf coordinate yields x = 0, hence i = 0, u = 0.
  struct SimTerrainCell
  {
    int i;
    double u;
  };
  SMPC_TERRAIN_FN SimTerrainCell sim_terrain_cell(double p, double o, double cell, int n)
  {
    const double hi = (double)(n - 1), im = (double)(n - 2);
    const double x = (p - o) / cell;
    const double lo = x > 0.0 ? x : 0.0;                               // (NaN, -0.0 and everything negative: +0.0)
    const double cl = lo < hi ? lo : hi;                               // (everything beyond the last node: n - 1)
    const double xc = fabs(x) <= 1.7976931348623157e308 ? cl : 0.0;    // (NaN and +-inf: 0)
    const double fl = floor(xc);
    const double fi = fl < im ? fl : im;
    SimTerrainCell r;
    r.i = (int)fi; // (fi is an integer in [0, n - 2])
    r.u = xc - fi;
    return r;
  }

  // height h, slopes and unit normal n of the bilinear patch with corner heights h00 (j, i), h10 (j, i + 1), h01 (j + 1, i), h11 at
  // fractions u (along x) and v (along y).  The order of operations makes a patch of equal heights z give h = z and n = (0, 0, 1) exactly.
  struct SimTerrainSample
  {
    double h, n[3];
  };
  SMPC_TERRAIN_FN SimTerrainSample sim_terrain_sample(double h00, double h10, double h01, double h11, double u, double v, double cell)
  {
    const double dx0 = h10 - h00, dx1 = h11 - h01, dy0 = h01 - h00;
    const double h0 = h00 + u * dx0, h1 = h01 + u * dx1;
    const double hx = (dx0 + v * (dx1 - dx0)) / cell;
    const double hy = (dy0 + u * ((h11 - h10) - dy0)) / cell;
    const double s = 1.0 / sqrt(hx * hx + hy * hy + 1.0);
    SimTerrainSample r;
    r.h = h0 + v * (h1 - h0);
    r.n[0] = (0.0 - hx) * s;
    r.n[1] = (0.0 - hy) * s;
    r.n[2] = s;
    return r;
  }

  // "" if this terrain is accepted for n robots, else one sentence that names the field and the first offending index.  A null terrain
  // (none: the plane) is accepted.  Nothing is allocated before this has answered; a refused call leaves the previous terrain in force.
  //   nx, ny >= 2 and tiles >= 1; tiles ny nx <= SIM_TERRAIN_MAX_NODES; cell finite and positive; heights non-null and finite; tile (may
  //   be null: 0) in [0, tiles); origin (may be null: (0, 0)) finite; hx^2 + hy^2 <= 3 at each of the four corners of every cell (the
  //   gradient of a bilinear patch is extremal at its corners).
  inline std::string sim_terrain_admission_error(int n, const smpc_terrain_settings * t)
  {
    char b[240];
    auto say = [&](const char * fmt, auto... a) {
      std::snprintf(b, sizeof(b), fmt, a...);
      return std::string("terrain: ") + b;
    };
    if (!t)
      return std::string();
    if (t->nx < 2)
      return say("nx = %d is below 2", t->nx);
    if (t->ny < 2)
      return say("ny = %d is below 2", t->ny);
    if (t->tiles < 1)
      return say("tiles = %d is below 1", t->tiles);
    if ((long long)t->tiles * t->ny * t->nx > SIM_TERRAIN_MAX_NODES)
      return say("tiles ny nx = %lld nodes is above the cap of %lld", (long long)t->tiles * t->ny * t->nx, SIM_TERRAIN_MAX_NODES);
    if (!std::isfinite(t->cell) || !(t->cell > 0.0))
      return say("cell = %g is not a positive finite number", t->cell);
    if (!t->heights)
      return say("heights is null");
    const int nx = t->nx, ny = t->ny;
    for (int k = 0; k < t->tiles; k++)
      for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++)
          if (!std::isfinite(t->heights[((size_t)k * ny + j) * nx + i]))
            return say("heights[%d][%d][%d] is not finite", k, j, i);
    if (t->tile)
      for (int r = 0; r < n; r++)
        if (t->tile[r] < 0 || t->tile[r] >= t->tiles)
          return say("tile[%d] = %d is outside [0, %d)", r, (int)t->tile[r], t->tiles);
    if (t->origin)
      for (int r = 0; r < n; r++)
        for (int k = 0; k < 2; k++)
          if (!std::isfinite(t->origin[(size_t)r * 2 + k]))
            return say("origin[%d][%d] is not finite", r, k);
    for (int k = 0; k < t->tiles; k++)
      for (int j = 0; j + 1 < ny; j++)
        for (int i = 0; i + 1 < nx; i++)
        {
          const double * H = t->heights + ((size_t)k * ny + j) * nx + i;
          const double h00 = H[0], h10 = H[1], h01 = H[nx], h11 = H[nx + 1];
          const double hx[2] = {(h10 - h00) / t->cell, (h11 - h01) / t->cell}, hy[2] = {(h01 - h00) / t->cell, (h11 - h10) / t->cell};
          for (int a = 0; a < 2; a++)
            for (int c = 0; c < 2; c++)
              if (!(hx[a] * hx[a] + hy[c] * hy[c] <= SIM_TERRAIN_MAX_SLOPE2))
                return say("slope[%d][%d][%d]: hx^2 + hy^2 = %g at a corner of the cell is above 3 (n.z below 0.5)", k, j, i, hx[a] * hx[a] + hy[c] * hy[c]);
        }
    return std::string();
  }
} // namespace smpc
