// smpc_id_rt_dims.h -- host-side sizes and admission of the inverse-dynamics QP on a RUN-TIME joint tree (smpc_id_rt.h): which engine a
// robot table goes to, the problem sizes of a point-foot and of a flat-foot robot, the ancestor sets of its joints.  Plain C++ with no backend
// behind it, so that stand-alone host programs can exercise it (tests/cpp/id_rt_dims_check.cpp, tests/cpp/id_rt6_dims_check.cpp).
#pragma once
#include "smpc_robot_check.h"
#include <vector>

namespace smpc
{
  constexpr int ID_RT_NFEET = 4;                        // point feet (tsid ContactPoint): 3 force variables, 3 motion rows, 4 friction rows each
  constexpr int ID_RT_MAX_NV = SMPC_MAX_JOINTS + 5;     // 37
  constexpr int ID_RT_MAX_N = ID_RT_MAX_NV + 3 * ID_RT_NFEET;   // 49 variables [a ; f]
  constexpr int ID_RT_MAX_GR = 6 + 7 * ID_RT_NFEET + ID_RT_MAX_NV - 6; // 65 general rows: dynamics | contact motion | friction | actuation

  struct IdRtSizes
  {
    int nq, nv, na, nf, n, m, np, mp, gr; // n = nv + 12 ; m = n + 6 + 12 + 16 + na ; padded to multiples of 16 ; gr = m - n
  };
  inline IdRtSizes id_rt_sizes(int njoints)
  {
    IdRtSizes s;
    s.nq = njoints + 6;
    s.nv = njoints + 5;
    s.na = s.nv - 6;
    s.nf = ID_RT_NFEET;
    s.n = s.nv + 3 * s.nf;
    s.m = s.n + 6 + 3 * s.nf + 4 * s.nf + s.na;
    s.np = ((s.n + 15) / 16) * 16;
    s.mp = ((s.m + 15) / 16) * 16;
    s.gr = s.m - s.n;
    return s;
  }

  enum IdRoute
  {
    ID_ROUTE_GO2 = 0,   // 13 joints / 4 point feet: IdEngine<FullGo2>
    ID_ROUTE_TALOS = 1, // 23 joints / 2 flat feet: IdEngine<FullTalos>
    ID_ROUTE_RT = 2,    // any other validated table with 4 point feet: IdEngineRt
    ID_ROUTE_REFUSED = 3,
    ID_ROUTE_RT6 = 4    // id_route_any only: any other validated table with 2 flat feet: IdEngineRt on its flat-foot kernels
  };
  // which engine smpc_id_create builds for a table; `why` receives the refusal.  force_rt: the debug switch that sends the built point-foot
  // shape through the run-time engine.  Nothing is allocated before this has answered.
  inline IdRoute id_route(const smpc_robot_model * rm, bool flat_feet, int go2_nj, int go2_nf, int talos_nj, int talos_nf, bool force_rt, std::string & why)
  {
    why.clear();
    if (!flat_feet && rm->njoints == go2_nj && rm->nfeet == go2_nf && !force_rt)
      return ID_ROUTE_GO2;
    if (flat_feet && rm->njoints == talos_nj && rm->nfeet == talos_nf)
      return ID_ROUTE_TALOS;
    if (flat_feet)
    {
      why = "the inverse-dynamics engine is instantiated for 13 joints / 4 point feet and for 23 joints / 2 flat feet; flat feet (force size 6) on "
            "a run-time joint tree are not built: only robots with 4 point feet (force size 3) go to the run-time engine";
      return ID_ROUTE_REFUSED;
    }
    why = robot_table_error(rm);
    if (!why.empty())
      return ID_ROUTE_REFUSED;
    if (rm->nfeet != ID_RT_NFEET)
    {
      char b[160];
      std::snprintf(b, sizeof(b), "robot table: nfeet = %d, the inverse-dynamics engine on a run-time joint tree is built for %d point feet", rm->nfeet, ID_RT_NFEET);
      why = b;
      return ID_ROUTE_REFUSED;
    }
    return ID_ROUTE_RT;
  }

  // ---- flat feet (tsid Contact6d) on a run-time joint tree: 2 feet, 12 corner-force variables, 6 LOCAL motion rows, 17 friction / bound rows each ----
  constexpr int ID_RT6_NFEET = 2;
  constexpr int ID_RT6_NFV = 12, ID_RT6_NM = 6, ID_RT6_NFR = 17;
  constexpr int ID_RT6_MAX_N = ID_RT_MAX_NV + ID_RT6_NFV * ID_RT6_NFEET;            // 61 variables [a ; corner forces]
  constexpr int ID_RT6_FR = ID_RT6_NFR * ID_RT6_NFEET;                              // 34 friction rows (closed form in the solver)
  constexpr int ID_RT6_MAX_DR = 6 + ID_RT6_NM * ID_RT6_NFEET + ID_RT_MAX_NV - 6;    // 49 dense general rows: dynamics | contact motion | actuation

  struct IdRt6Sizes
  {
    int nq, nv, na, nf, n, m, np, mp, gr, dr, fr; // n = nv + 24 ; m = n + 6 + 12 + 34 + na ; padded to multiples of 16 ; gr = m - n = dr + fr
  };
  inline IdRt6Sizes id_rt6_sizes(int njoints)
  {
    IdRt6Sizes s;
    s.nq = njoints + 6;
    s.nv = njoints + 5;
    s.na = s.nv - 6;
    s.nf = ID_RT6_NFEET;
    s.n = s.nv + ID_RT6_NFV * s.nf;
    s.dr = 6 + ID_RT6_NM * s.nf + s.na;
    s.fr = ID_RT6_FR;
    s.m = s.n + s.dr + s.fr;
    s.np = ((s.n + 15) / 16) * 16;
    s.mp = ((s.m + 15) / 16) * 16;
    s.gr = s.m - s.n;
    return s;
  }

  // which engine smpc_id_create_any builds: id_route for every input but one -- flat feet on a shape that is not the built one (or on the
  // built one under force_rt) go to the run-time flat-foot engine, once robot_table_error has accepted the table and it has 2 feet.
  // Nothing is allocated before this has answered.
  inline IdRoute id_route_any(const smpc_robot_model * rm, bool flat_feet, int go2_nj, int go2_nf, int talos_nj, int talos_nf, bool force_rt, std::string & why)
  {
    const bool built = rm->njoints == talos_nj && rm->nfeet == talos_nf;
    if (!flat_feet || (built && !force_rt))
      return id_route(rm, flat_feet, go2_nj, go2_nf, talos_nj, talos_nf, force_rt, why);
    why = robot_table_error(rm);
    if (!why.empty())
      return ID_ROUTE_REFUSED;
    if (rm->nfeet != ID_RT6_NFEET)
    {
      char b[200];
      std::snprintf(b, sizeof(b), "robot table: nfeet = %d, the inverse-dynamics engine for flat feet (force size 6) on a run-time joint tree is built for %d flat feet",
                    rm->nfeet, ID_RT6_NFEET);
      why = b;
      return ID_ROUTE_REFUSED;
    }
    return ID_ROUTE_RT6;
  }

  // limit vectors of the actuated joints: nv - 6 entries each
  inline std::string id_limits_error(int na, size_t n_tau, size_t n_v, size_t n_qmin, size_t n_qmax)
  {
    const size_t want = (size_t)na;
    const char * names[4] = {"effort_limit", "velocity_limit", "q_min", "q_max"};
    const size_t got[4] = {n_tau, n_v, n_qmin, n_qmax};
    for (int i = 0; i < 4; i++)
      if (got[i] != want)
      {
        char b[160];
        std::snprintf(b, sizeof(b), "inverse-dynamics settings: %s has %zu entries, expected nv - 6 = %d", names[i], got[i], na);
        return b;
      }
    return std::string();
  }

  // anc[j]: bit k set when joint k lies on the path from the root to joint j (j itself included); the table has passed robot_table_error
  inline std::vector<unsigned> id_rt_ancestors(const smpc_robot_model * rm)
  {
    std::vector<unsigned> anc((size_t)SMPC_MAX_JOINTS, 0u);
    const int nj = rm->njoints < SMPC_MAX_JOINTS ? rm->njoints : SMPC_MAX_JOINTS;
    for (int j = 0; j < nj; j++)
    {
      const int p = j == 0 ? -1 : rm->parent[j];
      anc[j] = (1u << j) | ((p >= 0 && p < j) ? anc[p] : 0u);
    }
    return anc;
  }
} // namespace smpc
