// smpc_sim_ground_joint_rt.h -- the ground of smpc_sim_ground_ws_rt.h with a JOINT MODEL: effort limits, implicit viscous damping,
// armature and joint-limit stops per robot (DESIGN 3.26 states the model word for word).  sim_ground_joint_rt_body is a sibling of
// sim_ground_ws_rt_body, which stays as it is: one wavefront per robot, one launch per step, the same phases with these additions
//   phase 0   the five joint arrays beside the torques, on the lanes that load the torques: tau is clipped to [-tau_max, tau_max] as it
//             is loaded (a NaN passes through), d, r_a + dt d, q_lo and q_hi go to LDS (null arrays: +inf, 0, 0, no limits)
//   inertia   Mh = M + diag(0_6, r_a + dt d) as M is formed; one lane walks the actuated joints in ascending order and lists the first
//             NJ = 8 stop candidates (joint, side, gap term), the rest are counted in `dropped`
//   phase 3   a stop row is a row of J behind the contact rows with the single entry s at column 6 + k
//   phase 4   the right-hand side loses d o v_joint; W, G, c0 and 1 / (dt G_rr) cover the stop rows as they cover the contact rows
//   phase 5   after the contact points of a sweep, the stop rows in ascending order on lane 0 (the update of a normal row); the dot
//             products of every row run over the whole row of the instantiation, so a stop and a foot see each other; rho takes the stop
//             rows too.  Stop rows start from exactly 0; the warm row holds contact rows only
//   phase 7   tau_applied, stop_rows, lam_stop and dropped with the other global stores
// NROWS counts contact rows AND stop rows: <24> serves up to 12 contact rows (5 points fit), <32> up to 24, each with 8 stop rows.
// With tau_max = +inf, d = r_a = 0 and stops = 0 every added term is an exact zero and the results equal the sibling's bit for bit.
// LDS: IdQuantRtScratch (19 024 B) + SimGroundJointLds<NROWS> = SimGroundWsLds<NROWS> + 4 (nv_max - 6) + 8 doubles + 18 ints.
// PER-ROBOT BODY PARAMETERS: sim_ground_body_rt_body<NROWS> is the same source compiled with BODY = true.  Its tree walk
// loads mass, com and inertia of body j of robot i from body[i][j][0..9] (global memory -> registers of lane j, in the walk's first phase)
// instead of from the device table; every other instruction is shared, the LDS is the same, and sim_ground_joint_rt_body compiles to
// what it compiled to before the flag existed.
// PER-ROBOT HEIGHT-FIELD TERRAIN: sim_ground_terrain_rt_body<NROWS> is the same source compiled with BODY and TERRAIN = true.
// Phase 0 also loads tile and origin of the robot; the point lanes of the phase that forms p_c sample the robot's tile below their point
// (four 8-byte loads per lane, issued together: THE ONE GLOBAL LOAD OUTSIDE PHASE 0, which cannot move there because its address depends
// on the forward kinematics) and form the point's own normal, frame and gap; phase 3 rotates each J entry and phase 7 each lambda by its
// point's frame, and phase 7 stores n_c and h of every point.  The per-point frames overlay sc.fb, dead after the tree walk: the LDS and
// its bounds are unchanged, and the four earlier entry points compile to what they compiled to before the flag existed.
// BODY POINTS: sim_ground_points_rt_body<32> / sim_ground_points_terrain_rt_body<32> are the same source compiled with
// POINTS = true (and BODY; TERRAIN for the second).  Phase 0 also loads joint and offset of body point k into the registers of lane k; the
// phase that forms p_c places the points on lanes 0 .. 15 (gap against the plane, or a terrain sample of their own: four more height loads
// on that lane, clamped as those of the feet), one lane then hands the candidates (phi_k < band, ascending k) the free slots behind the
// foot points, and the candidate lanes write position, gap and frame of their slot.  From phase 3 on a slot is a contact point whose joint
// is joint[k]; phase 7 stores body_slots, lam_body, body_gap, body_dropped and the touch byte.  The candidates' scratch lies in sc.fb
// behind the per-point frames: no LDS is added, and the six earlier entry points compile to what they compiled to before the flag existed.
#pragma once
#include "smpc_sim_ground_ws_rt.h"
#include "smpc_sim_joint_dims.h"
#include "smpc_sim_body_dims.h"
#include "smpc_sim_terrain_dims.h"
#include "smpc_sim_points_dims.h"
#include <vector>

namespace smpc
{
  struct SimGroundJointArgs
  {
    SimGroundWsArgs w;      // (sweeps_out / resid_out may be null here)
    const double * tau_max;  // [na] or [n][na] (device), or null: +inf
    const double * damping;  // or null: 0
    const double * armature; // or null: 0
    const double * q_lo;     // or null: -inf
    const double * q_hi;     // or null: +inf
    int per_robot, stops;
    double activation, stop_erp;
    double * tau_out;  // [n][na] or null
    int * rows_out;    // [n][NJ] or null
    double * lams_out; // [n][NJ] or null
    int * dropped_out; // [n] or null
  };

  template <int NROWS>
  struct SimGroundJointLds
  {
    static constexpr int NA = SIM_RT_MAX_NV - 6, NJ = SIM_JOINT_MAX_STOPS;
    SimGroundWsLds<NROWS> w;
    double dmp[NA], rad[NA], qlo[NA], qhi[NA]; // d, r_a + dt d, limits
    double sg[NJ];                             // g / dt or stop_erp g / dt of a stop row
    int sk[NJ], ss[NJ];                        // its joint and its side (+1 lower, -1 upper)
    int cnt[2];                                // rows, dropped
  };
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundJointLds<24>) <= 163840 / 3, "three blocks per compute unit");
  static_assert(sizeof(IdQuantRtScratch) + sizeof(SimGroundJointLds<32>) <= 163840 / 2, "two blocks per compute unit");

  // the terrain of a launch: device arrays and the dims of smpc_terrain_settings, and the two read-outs
  struct SimTerrainDev
  {
    const double * heights; // [tiles][ny][nx]
    const int * tile;       // [n] or null: 0
    const double * origin;  // [n][2] or null: (0, 0)
    int nx, ny, tiles;
    double cell;
    double * n_out; // [n][points][3] or null
    double * h_out; // [n][points] or null
  };

  // the body points of a launch: the device copy of smpc_body_points_settings with the band resolved, and the five read-outs
  struct SimPointsDev
  {
    const int * joint;     // [16]
    const double * offset; // [16][3]
    int n;
    double band;
    int * slots_out;           // [n][8] or null
    double * lam_out;          // [n][8][3] or null
    double * gap_out;          // [n][16] or null
    int * dropped_out;         // [n] or null
    unsigned char * touch_out; // [n] or null
  };

  // phi, h, and the frame t1 | t2 | n of the terrain below p (steps 1 - 6 of DESIGN 3.28: the sampling of the foot points, for a body point)
  struct SimPointSample
  {
    double phi, h, fr[9];
  };
  SMPC_DEV SimPointSample sim_points_terrain_sample(const SimTerrainDev * tr, const double ox, const double oy, const double td, const V3 p)
  {
    const int tnx = tr->nx > 2 ? tr->nx : 2, tny = tr->ny > 2 ? tr->ny : 2, tlast = tr->tiles > 1 ? tr->tiles - 1 : 0;
    const int tl = td < (double)tlast ? (td > 0.0 ? (int)td : 0) : tlast;
    const SimTerrainCell cx = sim_terrain_cell(p.x, ox, tr->cell, tnx), cy = sim_terrain_cell(p.y, oy, tr->cell, tny);
    const double * H = tr->heights + ((size_t)tl * tny + cy.i) * tnx + cx.i;
    const double h00 = H[0], h10 = H[1], h01 = H[tnx], h11 = H[tnx + 1]; // (the height loads of a body point, issued together)
    const SimTerrainSample sm = sim_terrain_sample(h00, h10, h01, h11, cx.u, cy.u, tr->cell);
    const double n0 = sm.n[0], n1 = sm.n[1], n2 = sm.n[2];
    const double fx = n2, fz = -n0;
    const double inv = 1.0 / sqrt(fx * fx + fz * fz);
    const V3 t1 = mk3(fx * inv, 0.0, fz * inv);
    SimPointSample r;
    st3(r.fr, t1);
    st3(r.fr + 3, mk3(n1 * t1.z - n2 * t1.y, n2 * t1.x - n0 * t1.z, n0 * t1.y - n1 * t1.x));
    st3(r.fr + 6, mk3(n0, n1, n2));
    r.h = sm.h;
    r.phi = n2 * (p.z - sm.h);
    return r;
  }

  // The one body of the step.  BODY = false is sim_ground_joint_rt_body; BODY = true is sim_ground_body_rt_body: `body` is
  // [n][nj][10] doubles on the device, and the tree walk of robot `inst` takes mass, com and inertia of body j from row [inst][j] instead
  // of from the device table (a null `body` reads the table; nj is the clamped joint count of the device table).  Nothing else differs.
  // TERRAIN = true is sim_ground_terrain_rt_body: every contact point has its own normal, frame and gap, sampled from the
  // robot's height-field tile below the point.  THE FOUR HEIGHT LOADS OF A POINT ARE THE ONE GLOBAL LOAD OUTSIDE PHASE 0, AND THEY CANNOT
  // MOVE THERE: their address depends on the point's position, which is the forward kinematics of the tree walk.  Each point lane issues
  // its four 8-byte loads together.  Every index is clamped in double before it becomes an integer (sim_terrain_cell), and the tile index
  // is clamped here, so no value read from memory can index outside `heights`.  env[0], env[1], env[2] carry origin x, origin y and the
  // tile of the robot (the plane is not read); the per-point frames t1 | t2 | n and the heights lie in sc.fb, which is dead once the tree
  // walk has formed the bias forces: no LDS is added.  With TERRAIN = false `tr` is not read and the code is what it was.
  // POINTS = true (NROWS = 32 only) adds the body points of `bp`: their candidates take the contact points npts .. npts + nb - 1
  // (the free slots), whose joint is joint[k] instead of fj[c / P].  sc.fb behind the frames holds, per body point, phi and its slot, and
  // per slot its point and its joint (small integers, exact in a double).  With POINTS = false `bp` is not read and the code is what it was.
  template <int NROWS, bool BODY, bool TERRAIN, bool POINTS>
  SMPC_DEV void sim_ground_joint_rt_impl(const SimGroundJointArgs & ja, const double * body, const SimTerrainDev * tr, const SimPointsDev * bp, int block)
  {
    typedef IdQuantRtScratch SC;
    typedef SimGroundLds<NROWS> L;
    typedef SimGroundEnvLds<NROWS> LE;
    typedef SimGroundWsLds<NROWS> LW;
    typedef SimGroundJointLds<NROWS> LJ;
    constexpr int NT = 64, MAXJ = SC::MAXJ, NF = SC::NF, LDM = L::NV, NCM = L::NC, NR = L::NR, LDG = L::LDG, NE = SIM_GROUND_ENV_DOUBLES, NJ = LJ::NJ,
                  NPM = (NROWS - NJ) / 3;
    static_assert(LDM <= NT - NE - 1 && NR <= NT && NCM <= 32 && NPM >= 1 && NPM <= L::NP && 3 * NPM + NJ <= NCM && NPM <= 24 && LDM - 6 <= LJ::NA,
                  "torques and environment load side by side; rows on lanes 32 .. 63; points on lanes 32 .. 55");
    const SimGroundWsArgs & wa = ja.w;
    const SimGroundEnvArgs & ea = wa.e;
    const SimGroundArgs & ka = ea.g;
    const int inst = block;
    const IdRtDevModel & mi = *ka.model;
    static_assert(!TERRAIN || 10 * NPM <= MAXJ * 6, "the per-point frames and heights overlay sc.fb");
    // sc.fb with body points: frames [9 NPM) | heights [NPM) | phi_k [16) | slot of k [16) | k of slot s [8) | joint of slot s [8) | slots in use, dropped
    constexpr int NBP = SIM_POINTS_MAX, NBS = SIM_POINTS_SLOTS, FB_PHI = 10 * NPM, FB_SLOT = FB_PHI + NBP, FB_K = FB_SLOT + NBP, FB_J = FB_K + NBS,
                  FB_CNT = FB_J + NBS;
    static_assert(!POINTS || (NROWS == 32 && NPM == NBS && FB_CNT + 2 <= MAXJ * 6 && NBP <= 32 && 3 * NBS <= 32),
                  "body points: the 32-row instantiation only; the candidates' scratch overlays sc.fb behind the frames; points on lanes 0 .. 15");
    // (wave-uniform sizes from the device table and the arguments, clamped so that no value can index outside the LDS arrays)
    const int nj = mi.t.njoints < MAXJ ? (mi.t.njoints > 1 ? mi.t.njoints : 1) : MAXJ;
    const int nv = nj + 5, nq = nj + 6, nx = 2 * nj + 11, na = nv - 6;
    const int P = ka.P < SIM_GROUND_MAX_PPF ? (ka.P > 1 ? ka.P : 1) : SIM_GROUND_MAX_PPF;
    const int maxf = NPM / P < NF ? NPM / P : NF;
    const int nfeet = mi.t.nfeet < maxf ? (mi.t.nfeet > 0 ? mi.t.nfeet : 0) : maxf;
    const int npts = nfeet * P, nr = 3 * npts;
    const int jpush = ea.push_joint < nj ? (ea.push_joint > 0 ? ea.push_joint : 0) : nj - 1;
    const double dt = ka.dt;
    const bool warm = wa.warm_start != 0 && wa.lam0 != nullptr;
    // (body points: the count and the free slots are wave-uniform and clamped; the values of point k live in the registers of lane k)
    const int nbp = POINTS ? (bp->n < NBP ? (bp->n > 0 ? bp->n : 0) : NBP) : 0;
    const int smax = POINTS ? NPM - npts : 0;
    SMPC_PL(int, bpj, NT);
    SMPC_PLA(double, bpv, NT, 16); // offset 0..2 -> p_k 0..2 | phi 3 | h 4 | frame 5..13
    SMPC_LDS(SC, scs, 1);
    SMPC_LDS(LJ, ls, 1);
    SC & sc = scs[0];
    LJ & jm = ls[0];
    LW & w = jm.w;
    LE & e = w.e;
    L & s = e.s;
    // ---- phase 0: every global load (the state and the joint constants: first phase of rt_tree_phases) ----
    SMPC_LANES(NT)
    {
      if (lane < LDM)
      {
        double t = 0.0;
        if (lane >= 6 && lane < nv)
        {
          const int k = lane - 6;
          const size_t at = (ja.per_robot != 0 ? (size_t)inst * na : (size_t)0) + k;
          t = ka.tau[(size_t)inst * na + k];
          const double tm = ja.tau_max != nullptr ? ja.tau_max[at] : INFINITY;
          const double d = ja.damping != nullptr ? ja.damping[at] : 0.0;
          const double ra = ja.armature != nullptr ? ja.armature[at] : 0.0;
          t = t > tm ? tm : (t < -tm ? -tm : t); // (a NaN passes through)
          jm.dmp[k] = d;
          jm.rad[k] = ra + dt * d;
          jm.qlo[k] = ja.q_lo != nullptr ? ja.q_lo[at] : -INFINITY;
          jm.qhi[k] = ja.q_hi != nullptr ? ja.q_hi[at] : INFINITY;
        }
        s.tau[lane] = t;
      }
      if (lane >= NT - NE)
      {
        const int k = lane - (NT - NE);
        double val;
        if (TERRAIN && k < 4) // origin x, origin y and the tile of the robot (an int32 is exact in a double; clamped where it is used)
          val = k < 2 ? (tr->origin != nullptr ? tr->origin[(size_t)inst * 2 + k] : 0.0) : (k == 2 && tr->tile != nullptr ? (double)tr->tile[inst] : 0.0);
        else if (k < 4)
          val = ea.plane != nullptr ? ea.plane[(size_t)inst * 4 + k] : (k == 2 ? 1.0 : (k == 3 ? ka.ground_z : 0.0));
        else if (k == 4)
          val = ea.mu != nullptr ? ea.mu[inst] : ka.mu;
        else
          val = ea.push != nullptr ? ea.push[(size_t)inst * 6 + k - 5] : 0.0;
        e.env[k] = val;
      }
      if (lane < NCM) // the start vector: the robot's warm row (contact rows only), an entry that is not finite reads as exactly 0
      {
        double val = 0.0;
        if (warm && lane < nr)
        {
          const double v = wa.lam0[(size_t)inst * nr + lane];
          val = fabs(v) <= 1.7976931348623157e308 ? v : 0.0;
        }
        s.lam[lane] = val;
      }
      if constexpr (POINTS)
      {
        const int k = lane < nbp ? lane : 0;
        int j = 0;
        double o0 = 0.0, o1 = 0.0, o2 = 0.0;
        if (nbp > 0) // (wave-uniform; the pointers are read only then)
        {
          j = bp->joint[k];
          o0 = bp->offset[k * 3];
          o1 = bp->offset[k * 3 + 1];
          o2 = bp->offset[k * 3 + 2];
        }
        SMPC_PLV(bpj) = j < nj ? (j > 0 ? j : 0) : nj - 1; // (clamped here as well: it indexes LDS)
        SMPC_PLV(bpv)[0] = o0;
        SMPC_PLV(bpv)[1] = o1;
        SMPC_PLV(bpv)[2] = o2;
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phases 1, 2 ----
    if constexpr (BODY) // (the pointer is null-checked once, wave-uniformly: it is a kernel argument)
      rt_tree_phases_impl<true>(sc, mi, ka.X + (size_t)inst * nx, mk3(ka.gravity[0], ka.gravity[1], ka.gravity[2]),
                                body != nullptr ? body + (size_t)inst * nj * 10 : nullptr);
    else
      rt_tree_phases(sc, mi, ka.X + (size_t)inst * nx, mk3(ka.gravity[0], ka.gravity[1], ka.gravity[2]));
    // ---- Mh = M + diag(0_6, r_a + dt d) (both triangles from one expression: symmetric bit for bit); contact points, gaps, frame and push
    // point; the stop candidates ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < nv * nv; idx += NT)
      {
        const int r = idx / nv, c = idx % nv;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const int jl = lo < 6 ? 0 : lo - 5, jh = hi < 6 ? 0 : hi - 5;
        double val = ((sc.anc[jh] >> jl) & 1u) ? id_rt_dot6(&sc.S[lo * 6], &sc.F[hi * 6]) : 0.0;
        if (r == c && r >= 6)
          val += jm.rad[r - 6];
        s.M[r * LDM + c] = val;
      }
      for (int idx = lane; idx < NCM * LDM; idx += NT)
        s.J[idx] = 0.0;
      if (lane < NCM)
      {
        s.c0[lane] = 0.0;
        w.ig[lane][0] = 0.0;
        w.ig[lane][1] = 0.0;
      }
      if (lane >= 32 && lane < 32 + NPM)
      {
        const int c = lane - 32;
        double gap = 0.0;
        V3 p = mk3(0.0, 0.0, 0.0);
        if (c < npts)
        {
          const int f = c / P, k = c % P, jf = sc.fj[f];
          p = ld3(&sc.footp[f * 3]) + ldm3(&sc.oR[jf * 9]) * mk3(ka.points[k][0], ka.points[k][1], ka.points[k][2]); // foot frame rotation = joint rotation
          if constexpr (TERRAIN)
          {
            const int tnx = tr->nx > 2 ? tr->nx : 2, tny = tr->ny > 2 ? tr->ny : 2, tlast = tr->tiles > 1 ? tr->tiles - 1 : 0;
            const double td = e.env[2];
            const int tl = td < (double)tlast ? (td > 0.0 ? (int)td : 0) : tlast;
            const SimTerrainCell cx = sim_terrain_cell(p.x, e.env[0], tr->cell, tnx), cy = sim_terrain_cell(p.y, e.env[1], tr->cell, tny);
            const double * H = tr->heights + ((size_t)tl * tny + cy.i) * tnx + cx.i;
            const double h00 = H[0], h10 = H[1], h01 = H[tnx], h11 = H[tnx + 1]; // (the one global load outside phase 0)
            const SimTerrainSample sm = sim_terrain_sample(h00, h10, h01, h11, cx.u, cy.u, tr->cell);
            // t1 = (e_y x n) / |e_y x n|, t2 = n x t1 (sim_ground_env_frame), of this point's normal
            const double n0 = sm.n[0], n1 = sm.n[1], n2 = sm.n[2];
            const double fx = n2, fz = -n0;
            const double inv = 1.0 / sqrt(fx * fx + fz * fz);
            const V3 t1 = mk3(fx * inv, 0.0, fz * inv);
            double * fr = &sc.fb[c * 9];
            st3(fr, t1);
            st3(fr + 3, mk3(n1 * t1.z - n2 * t1.y, n2 * t1.x - n0 * t1.z, n0 * t1.y - n1 * t1.x));
            st3(fr + 6, mk3(n0, n1, n2));
            sc.fb[9 * NPM + c] = sm.h;
            gap = n2 * (p.z - sm.h);
          }
          else
          {
            double acc = e.env[0] * p.x;
            acc += e.env[1] * p.y;
            acc += e.env[2] * p.z;
            gap = acc - e.env[3];
          }
        }
        st3(&s.pc[c * 3], p);
        s.gap[c] = gap;
      }
      if constexpr (POINTS)
        if (lane < nbp) // body point k on lane k: p_k = p_j + R_j o_k, its gap and, on a terrain, its own frame and height
        {
          const int j = SMPC_PLV(bpj);
          const V3 p = ld3(&sc.op[j * 3]) + ldm3(&sc.oR[j * 9]) * mk3(SMPC_PLV(bpv)[0], SMPC_PLV(bpv)[1], SMPC_PLV(bpv)[2]);
          double phi;
          if constexpr (TERRAIN)
          {
            const SimPointSample sm = sim_points_terrain_sample(tr, e.env[0], e.env[1], e.env[2], p);
            phi = sm.phi;
            SMPC_PLV(bpv)[4] = sm.h;
#pragma unroll
            for (int i = 0; i < 9; i++)
              SMPC_PLV(bpv)[5 + i] = sm.fr[i];
          }
          else
          {
            double acc = e.env[0] * p.x;
            acc += e.env[1] * p.y;
            acc += e.env[2] * p.z;
            phi = acc - e.env[3];
          }
          SMPC_PLV(bpv)[0] = p.x;
          SMPC_PLV(bpv)[1] = p.y;
          SMPC_PLV(bpv)[2] = p.z;
          SMPC_PLV(bpv)[3] = phi;
          sc.fb[FB_PHI + lane] = phi;
        }
      if (lane == 60) // stop candidates in ascending k: min(g-, g+) < activation; lower if g- <= g+
      {
        int rows = 0, dropped = 0;
        if (ja.stops != 0)
          for (int k = 0; k < na; k++)
          {
            const double q = sc.x[7 + k];
            const double gm = q - jm.qlo[k], gp = jm.qhi[k] - q;
            const bool lower = gm <= gp;
            const double g = lower ? gm : gp;
            if (g < ja.activation)
            {
              if (rows < NJ)
              {
                jm.sk[rows] = k;
                jm.ss[rows] = lower ? 1 : -1;
                jm.sg[rows] = g >= 0.0 ? g / dt : ja.stop_erp * g / dt;
                rows++;
              }
              else
                dropped++;
            }
          }
        for (int r = rows; r < NJ; r++)
        {
          jm.sk[r] = 0;
          jm.ss[r] = 0;
          jm.sg[r] = 0.0;
        }
        jm.cnt[0] = rows;
        jm.cnt[1] = dropped;
      }
      if (!TERRAIN && lane == 62) // t1 = (e_y x n) / |e_y x n|, t2 = n x t1 (sim_ground_env_frame)
      {
        const double n0 = e.env[0], n1 = e.env[1], n2 = e.env[2];
        const double cx = n2, cz = -n0;
        const double inv = 1.0 / sqrt(cx * cx + cz * cz);
        const V3 t1 = mk3(cx * inv, 0.0, cz * inv);
        st3(e.t1, t1);
        st3(e.t2, mk3(n1 * t1.z - n2 * t1.y, n2 * t1.x - n0 * t1.z, n0 * t1.y - n1 * t1.x));
      }
      if (lane == 63) // r = p_j + R_j o and r x f
      {
        const V3 r = ld3(&sc.op[jpush * 3]) + ldm3(&sc.oR[jpush * 9]) * ld3(&e.env[8]);
        st3(e.r, r);
        st3(e.rxf, cross(r, ld3(&e.env[5])));
      }
    }
    SMPC_LANES_END_WAVE
    int nb_raw = 0, nb_drop = 0;
    if constexpr (POINTS)
    {
      // one lane walks the body points in ascending k: phi_k < band (a NaN is none) takes the next free slot, the rest are counted
      SMPC_LANES(NT)
      if (lane == 61)
      {
        int used = 0, dropped = 0;
        for (int k = 0; k < nbp; k++)
        {
          int slot = -1;
          if (sc.fb[FB_PHI + k] < bp->band)
          {
            if (used < smax)
            {
              slot = used;
              sc.fb[FB_K + used] = (double)k;
              used++;
            }
            else
              dropped++;
          }
          sc.fb[FB_SLOT + k] = (double)slot;
        }
        for (int r = used; r < NBS; r++)
          sc.fb[FB_K + r] = 0.0;
        sc.fb[FB_CNT] = (double)used;
        sc.fb[FB_CNT + 1] = (double)dropped;
      }
      SMPC_LANES_END_WAVE
      // the candidate lanes write their slot: contact point npts + slot
      SMPC_LANES(NT)
      {
        if (lane >= 32 && lane < 32 + NBS)
          sc.fb[FB_J + lane - 32] = 0.0;
        if (lane < nbp)
        {
          const int slot = (int)sc.fb[FB_SLOT + lane];
          if (slot >= 0 && slot < smax)
          {
            const int c = npts + slot;
            st3(&s.pc[c * 3], mk3(SMPC_PLV(bpv)[0], SMPC_PLV(bpv)[1], SMPC_PLV(bpv)[2]));
            s.gap[c] = SMPC_PLV(bpv)[3];
            if constexpr (TERRAIN)
            {
#pragma unroll
              for (int i = 0; i < 9; i++)
                sc.fb[c * 9 + i] = SMPC_PLV(bpv)[5 + i];
              sc.fb[9 * NPM + c] = SMPC_PLV(bpv)[4];
            }
          }
        }
      }
      SMPC_LANES_END_WAVE
      SMPC_LANES(NT)
      if (lane < nbp)
      {
        const int slot = (int)sc.fb[FB_SLOT + lane];
        if (slot >= 0 && slot < smax)
          sc.fb[FB_J + slot] = (double)SMPC_PLV(bpj);
      }
      SMPC_LANES_END_WAVE
      nb_raw = (int)SMPC_UNIFORM_U32((int)sc.fb[FB_CNT]);
      nb_drop = (int)SMPC_UNIFORM_U32((int)sc.fb[FB_CNT + 1]);
    }
    // (wave-uniform: one wavefront owns one robot; clamped before it indexes anything)
    const int nb = POINTS ? (nb_raw < smax ? (nb_raw > 0 ? nb_raw : 0) : (smax > 0 ? smax : 0)) : 0;
    const int npt = npts + nb, nrp = 3 * npt; // contact points and rows with the slots in use (npts and nr without body points)
    const int ns_raw = (int)SMPC_UNIFORM_U32(jm.cnt[0]);
    const int ns_max = NCM - nrp < NJ ? NCM - nrp : NJ;
    const int ns = ns_raw < ns_max ? (ns_raw > 0 ? ns_raw : 0) : ns_max;
    const int nrt = nrp + ns;
    // ---- phase 3: the rows of every point, t1 t2 n in the contact frame; the stop rows behind them ----
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < npt * nv; idx += NT)
      {
        const int c = idx / nv, k = idx % nv;
        int jf;
        if (POINTS && c >= npts) // (a slot: the joint of its body point, clamped again as it comes from LDS)
        {
          const int jb = (int)sc.fb[FB_J + c - npts];
          jf = jb < nj ? (jb > 0 ? jb : 0) : nj - 1;
        }
        else
          jf = sc.fj[c / P];
        const int jk = k < 6 ? 0 : k - 5;
        if ((sc.anc[jf] >> jk) & 1u)
        {
          const SV Sk = ldsv(&sc.S[k * 6]);
          const V3 lin = Sk.l + cross(Sk.a, ld3(&s.pc[c * 3])); // velocity of the point under the unit twist of column k
          const double *ft1 = TERRAIN ? &sc.fb[c * 9] : e.t1, *ft2 = TERRAIN ? &sc.fb[c * 9 + 3] : e.t2, *fn = TERRAIN ? &sc.fb[c * 9 + 6] : e.env;
          double r0 = ft1[0] * lin.x;
          r0 += ft1[1] * lin.y;
          r0 += ft1[2] * lin.z;
          double r1 = ft2[0] * lin.x;
          r1 += ft2[1] * lin.y;
          r1 += ft2[2] * lin.z;
          double r2 = fn[0] * lin.x;
          r2 += fn[1] * lin.y;
          r2 += fn[2] * lin.z;
          s.J[(3 * c + 0) * LDM + k] = r0;
          s.J[(3 * c + 1) * LDM + k] = r1;
          s.J[(3 * c + 2) * LDM + k] = r2;
        }
      }
      if (lane >= 32 && lane < 32 + ns) // (other lanes than the ones that write the rows of the points: J_r = s e_{6 + k})
      {
        const int r = lane - 32;
        const int k = jm.sk[r] < na ? (jm.sk[r] > 0 ? jm.sk[r] : 0) : na - 1;
        s.J[(nrp + r) * LDM + 6 + k] = (double)jm.ss[r];
      }
    }
    SMPC_LANES_END_WAVE
    // ---- phase 4: Mh = L L^T ; W = Mh^-1 [S tc - h - d o v + Q | J^T] ----
    SMPC_LANES(NT)
    for (int idx = lane; idx < nv * NR; idx += NT)
    {
      const int k = idx / NR, c = idx % NR;
      double val;
      if (c == 0)
      {
        double q = 0.0;
        if ((sc.anc[jpush] >> (k < 6 ? 0 : k - 5)) & 1u)
        {
          const SV Sk = ldsv(&sc.S[k * 6]);
          q = Sk.l.x * e.env[5];
          q += Sk.l.y * e.env[6];
          q += Sk.l.z * e.env[7];
          q += Sk.a.x * e.rxf[0];
          q += Sk.a.y * e.rxf[1];
          q += Sk.a.z * e.rxf[2];
        }
        val = s.tau[k] - sc.h[k];
        if (k >= 6)
          val -= jm.dmp[k - 6] * sc.x[nq + k];
        val += q;
      }
      else
        val = s.J[(c - 1) * LDM + k];
      s.W[idx] = val;
    }
    SMPC_LANES_END_WAVE
    rt_wave_cholesky(s.M, LDM, nv, s.tmp);
    rt_wave_chol_solve<NR>(s.M, LDM, nv, s.W, NR, s.row);
    // free velocity
    SMPC_LANES(NT)
    if (lane < nv)
      s.vf[lane] = sc.x[nq + lane] + dt * s.W[lane * NR];
    SMPC_LANES_END_WAVE
    // Delassus matrix with the compliance on its diagonal, c0 = J v_f + the gap term on the normal rows and on the stop rows
    SMPC_LANES(NT)
    {
      for (int idx = lane; idx < NCM * NCM; idx += NT)
      {
        const int c = idx / NCM, d = idx % NCM;
        double acc = 0.0;
        if (c < nrt && d < nrt) // (zero beyond the robot's rows: the sweep runs over the whole row)
        {
          for (int k = 0; k < nv; k++)
            acc += s.J[c * LDM + k] * s.W[k * NR + 1 + d];
          if (c == d)
            acc += ka.compliance;
        }
        s.G[c * LDG + d] = acc;
      }
      if (lane >= 32 && lane < 32 + nrt)
      {
        const int r = lane - 32;
        double acc = 0.0;
        if (r < nrp)
        {
          for (int k = 0; k < nv; k++)
            acc += s.J[r * LDM + k] * s.vf[k];
          if (r % 3 == 2)
          {
            const double phi = s.gap[r / 3];
            acc += phi >= 0.0 ? phi / dt : ka.erp * phi / dt;
          }
        }
        else
        {
          const int i = r - nrp;
          const int k = jm.sk[i] < na ? (jm.sk[i] > 0 ? jm.sk[i] : 0) : na - 1;
          acc = (double)jm.ss[i] * s.vf[6 + k] + jm.sg[i];
        }
        s.c0[r] = acc;
      }
    }
    SMPC_LANES_END_WAVE
    SMPC_LANES(NT)
    if (lane < nrt)
    {
      const double dg = dt * s.G[lane * LDG + lane];
      w.ig[lane][0] = 1.0 / dg;
      w.ig[lane][1] = dg;
    }
    SMPC_LANES_END_WAVE
    // ---- phase 5: projected Gauss-Seidel from the start vector: the points in ascending order (the sweep of sim_ground_ws_rt_body), then
    // the stop rows in ascending order; at most `sweeps` sweeps; rho of a sweep on lanes 0 and 1, the stopping test once per sweep ----
    const int min_sweeps = wa.min_sweeps > 1 ? wa.min_sweeps : 1;
    const bool stopping = wa.tol > 0.0;
    int used = 0;
    double rho = 0.0;
    SMPC_PL(double, rmax, NT);
    SMPC_PL(double, tdg, NT); // dt G_rr of the lane's tangential row, from the phase of the candidates to the projection
    SMPC_LANES(NT)
    {
      SMPC_PLV(rmax) = 0.0;
      SMPC_PLV(tdg) = 0.0;
    }
    SMPC_LANES_END_WAVE
    for (int sw = 0; sw < ka.sweeps; sw++)
    {
      for (int c = 0; c < npt; c++)
      {
        const int rn = 3 * c + 2;
        SMPC_LANES(NT)
        if (lane == 0)
        {
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < NCM; j++) // (compile-time bound: the loads of the row are issued ahead of the chain of multiply-adds)
            acc += s.G[rn * LDG + j] * s.lam[j];
          const double old = s.lam[rn];
          const double idg = w.ig[rn][0], dg = w.ig[rn][1];
          const double val = fmax(0.0, old - (s.c0[rn] + dt * acc) * idg);
          s.lam[rn] = val;
          SMPC_PLV(rmax) = sim_ground_ws_max(SMPC_PLV(rmax), fabs(val - old) * dg);
        }
        SMPC_LANES_END_WAVE
        // both tangential candidates from the same lambda, the one that already holds the new normal force
        SMPC_LANES(NT)
        if (lane < 2)
        {
          const int rt = 3 * c + lane;
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < NCM; j++)
            acc += s.G[rt * LDG + j] * s.lam[j];
          const double idg = w.ig[rt][0];
          SMPC_PLV(tdg) = w.ig[rt][1];
          s.tc[lane] = s.lam[rt] - (s.c0[rt] + dt * acc) * idg;
        }
        SMPC_LANES_END_WAVE
        SMPC_LANES(NT)
        if (lane < 2)
        {
          const int rt = 3 * c + lane;
          const double t1 = s.tc[0], t2 = s.tc[1];
          const double nrm = sqrt(t1 * t1 + t2 * t2), lim = e.env[4] * s.lam[rn];
          const double old = s.lam[rt];
          double t = s.tc[lane];
          if (nrm > lim)
            t = t * (lim / nrm);
          if (nrm == 0.0)
            t = 0.0;
          s.lam[rt] = t;
          SMPC_PLV(rmax) = sim_ground_ws_max(SMPC_PLV(rmax), fabs(t - old) * SMPC_PLV(tdg));
        }
        SMPC_LANES_END_WAVE
      }
      for (int r = nrp; r < nrt; r++) // the stop rows: the update of a normal row
      {
        SMPC_LANES(NT)
        if (lane == 0)
        {
          double acc = 0.0;
#pragma unroll
          for (int j = 0; j < NCM; j++)
            acc += s.G[r * LDG + j] * s.lam[j];
          const double old = s.lam[r];
          const double idg = w.ig[r][0], dg = w.ig[r][1];
          const double val = fmax(0.0, old - (s.c0[r] + dt * acc) * idg);
          s.lam[r] = val;
          SMPC_PLV(rmax) = sim_ground_ws_max(SMPC_PLV(rmax), fabs(val - old) * dg);
        }
        SMPC_LANES_END_WAVE
      }
      SMPC_LANES(NT)
      if (lane < 2)
      {
        w.rho[lane] = SMPC_PLV(rmax);
        SMPC_PLV(rmax) = 0.0; // (the next sweep's maximum starts at 0)
      }
      SMPC_LANES_END_WAVE
      // (the whole wave reads the two maxima back: after the lanes' end-of-wave point, so that the sequential test backend sees both)
      rho = sim_ground_ws_max(w.rho[0], w.rho[1]);
      used = sw + 1;
      if (SMPC_UNIFORM_U32(stopping && used >= min_sweeps && rho <= wa.tol ? 1u : 0u) != 0u)
        break;
    }
    // ---- phase 6: a = W_0 + W_1 lambda ; v+ = v_f + dt W_1 lambda ; q+ = q (+) v+ dt ----
    SMPC_LANES(NT)
    if (lane < nv)
    {
      double acc = 0.0;
      for (int c = 0; c < nrt; c++)
        acc += s.W[lane * NR + 1 + c] * s.lam[c];
      s.a[lane] = s.W[lane * NR] + acc;
      const double vn = s.vf[lane] + dt * acc;
      s.xn[nq + lane] = vn;
      s.dx[lane] = vn * dt;
    }
    SMPC_LANES_END_WAVE
    const bool step = ka.advance != 0;
    if (step)
    {
      SMPC_LANES(NT)
      if (lane == 0)
      {
        const double * x = sc.x;
        const V3 dv = ld3(s.dx), dw = ld3(s.dx + 3);
        const M3 R0 = quat_to_R(Quat{x[3], x[4], x[5], x[6]});
        const SE3 E = exp6(dv, dw);
        st3(s.xn, ld3(x) + R0 * E.p);
        Quat qn = quat_mul(Quat{x[3], x[4], x[5], x[6]}, quat_exp(dw));
        const double n = 1.0 / sqrt(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);
        s.xn[3] = qn.x * n;
        s.xn[4] = qn.y * n;
        s.xn[5] = qn.z * n;
        s.xn[6] = qn.w * n;
      }
      else if (lane >= 6 && lane < nv)
        s.xn[lane + 1] = sc.x[lane + 1] + s.dx[lane];
      SMPC_LANES_END_WAVE
    }
    // ---- phase 7: every global store; the forces in world axes, lambda_world(c) = Rc lambda_c, and in the contact frame ----
    SMPC_LANES(NT)
    {
      if (step)
        for (int i = lane; i < nx; i += NT)
          ka.X[(size_t)inst * nx + i] = s.xn[i];
      if (lane < nv)
      {
        ka.a_out[(size_t)inst * nv + lane] = s.a[lane];
        if (ka.vnext_out != nullptr)
          ka.vnext_out[(size_t)inst * nv + lane] = s.xn[nq + lane];
      }
      if (lane < na && ja.tau_out != nullptr)
        ja.tau_out[(size_t)inst * na + lane] = s.tau[6 + lane];
      if (lane < nr)
      {
        const int c = lane / 3, i = lane % 3;
        const double *ft1 = TERRAIN ? &sc.fb[c * 9] : e.t1, *ft2 = TERRAIN ? &sc.fb[c * 9 + 3] : e.t2, *fn = TERRAIN ? &sc.fb[c * 9 + 6] : e.env;
        double wl = ft1[i] * s.lam[3 * c];
        wl += ft2[i] * s.lam[3 * c + 1];
        wl += fn[i] * s.lam[3 * c + 2];
        ka.lam_out[(size_t)inst * nr + lane] = wl;
        if constexpr (TERRAIN)
          if (tr->n_out != nullptr)
            tr->n_out[(size_t)inst * nr + lane] = fn[i];
        if (wa.lamc_out != nullptr)
          wa.lamc_out[(size_t)inst * nr + lane] = s.lam[lane];
      }
      if (lane < npts && ka.gap_out != nullptr)
        ka.gap_out[(size_t)inst * npts + lane] = s.gap[lane];
      if constexpr (TERRAIN)
        if (lane < npts && tr->h_out != nullptr)
          tr->h_out[(size_t)inst * npts + lane] = sc.fb[9 * NPM + lane];
      if (lane >= 32 && lane < 32 + NJ)
      {
        const int r = lane - 32;
        if (ja.rows_out != nullptr)
          ja.rows_out[(size_t)inst * NJ + r] = r < ns ? jm.ss[r] * (jm.sk[r] + 1) : 0;
        if (ja.lams_out != nullptr)
          ja.lams_out[(size_t)inst * NJ + r] = r < ns ? s.lam[nrp + r] : 0.0;
      }
      if (lane == 0)
      {
        unsigned word = 0u;
        for (int c = 0; c < npt; c++)
          if (s.lam[3 * c + 2] > 0.0)
            word |= 1u << c;
        ka.contact_out[inst] = word;
      }
      if constexpr (POINTS)
      {
        if (lane < 3 * NBS && bp->lam_out != nullptr) // lambda_world of slot lane / 3, 0 for a slot not in use
        {
          const int sl = lane / 3, i = lane % 3, c = npts + sl;
          double wl = 0.0;
          if (sl < nb)
          {
            const double *ft1 = TERRAIN ? &sc.fb[c * 9] : e.t1, *ft2 = TERRAIN ? &sc.fb[c * 9 + 3] : e.t2, *fn = TERRAIN ? &sc.fb[c * 9 + 6] : e.env;
            wl = ft1[i] * s.lam[3 * c];
            wl += ft2[i] * s.lam[3 * c + 1];
            wl += fn[i] * s.lam[3 * c + 2];
          }
          bp->lam_out[(size_t)inst * 3 * NBS + lane] = wl;
        }
        if (lane >= 32 && lane < 32 + NBS && bp->slots_out != nullptr)
        {
          const int r = lane - 32;
          bp->slots_out[(size_t)inst * NBS + r] = r < nb ? (int)sc.fb[FB_K + r] + 1 : 0;
        }
        if (lane >= 40 && lane < 40 + NBP && bp->gap_out != nullptr)
        {
          const int k = lane - 40;
          bp->gap_out[(size_t)inst * NBP + k] = k < nbp ? sc.fb[FB_PHI + k] : 0.0;
        }
        if (lane == 3 && bp->dropped_out != nullptr)
          bp->dropped_out[inst] = nb_drop + (nb_raw > nb ? nb_raw - nb : 0);
        if (lane == 4 && bp->touch_out != nullptr)
        {
          unsigned char touch = 0;
          for (int sl = 0; sl < nb; sl++)
            if (s.lam[3 * (npts + sl) + 2] > 0.0)
              touch = 1;
          bp->touch_out[inst] = touch;
        }
      }
      if (lane == 1)
      {
        if (wa.sweeps_out != nullptr)
          wa.sweeps_out[inst] = used;
        if (wa.resid_out != nullptr)
          wa.resid_out[inst] = rho;
      }
      if (lane == 2 && ja.dropped_out != nullptr)
        ja.dropped_out[inst] = jm.cnt[1] + (ns_raw > ns ? ns_raw - ns : 0);
    }
    SMPC_LANES_END_WAVE
  }

  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_joint_rt_body(const SimGroundJointArgs & ja, int block)
  {
    sim_ground_joint_rt_impl<NROWS, false, false, false>(ja, nullptr, nullptr, nullptr, block);
  }

  // ---- per-robot body parameters: the same step with the masses, centres of mass and inertias of robot i from body[i] ----
  struct SimGroundBodyArgs
  {
    SimGroundJointArgs j;
    const double * body; // [n][nj][10] (device): mass | com | Ixx Ixy Iyy Ixz Iyz Izz of every body, or null: the device table
  };
  // (no LDS of its own: the rows go from global memory to the registers of lane j, so the bounds asserted above hold unchanged)
  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_body_rt_body(const SimGroundBodyArgs & ba, int block)
  {
    sim_ground_joint_rt_impl<NROWS, true, false, false>(ba.j, ba.body, nullptr, nullptr, block);
  }

  // ---- per-robot height-field terrain: the same step with the normal, frame and gap of every contact point sampled from the
  // robot's tile; the body pointer is null-checked as above (null reads the table) ----
  struct SimGroundTerrainArgs
  {
    SimGroundBodyArgs b;
    SimTerrainDev t;
  };
  // (no LDS of its own: the frames overlay an array of the tree walk, so the bounds asserted above hold unchanged)
  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_terrain_rt_body(const SimGroundTerrainArgs & ta, int block)
  {
    sim_ground_joint_rt_impl<NROWS, true, true, false>(ta.b.j, ta.b.body, &ta.t, nullptr, block);
  }

  // ---- body points: the same step with contact candidates on any link in the free slots behind the foot points, and the
  // touch byte; on the plane and on the terrain.  The body pointer is null-checked as above (null reads the table).  NROWS = 32 only. ----
  struct SimGroundPointsArgs
  {
    SimGroundTerrainArgs t; // (t.t is not read on the plane)
    SimPointsDev p;
  };
  // (no LDS of their own: the candidates' scratch overlays the same array of the tree walk, so the bounds asserted above hold unchanged)
  // grid = n, 64 lanes
  template <int NROWS>
  SMPC_DEV void sim_ground_points_rt_body(const SimGroundPointsArgs & pa, int block)
  {
    sim_ground_joint_rt_impl<NROWS, true, false, true>(pa.t.b.j, pa.t.b.body, nullptr, &pa.p, block);
  }
  template <int NROWS>
  SMPC_DEV void sim_ground_points_terrain_rt_body(const SimGroundPointsArgs & pa, int block)
  {
    sim_ground_joint_rt_impl<NROWS, true, true, true>(pa.t.b.j, pa.t.b.body, &pa.t.t, &pa.p, block);
  }

  // ---- host: the joint model and the per-robot read-outs of one simulator handle's ground (a sibling of RobotSimGroundWs; the
  // environment and the solver state of a step are handed in by the caller).  `active` once the setter has been called: from then on the
  // handle's ground steps launch the kernel above.  The host-buffer solve needs no setter, allocates its staging only and never touches the
  // handle's buffers. ----
  struct RobotSimGroundJoint
  {
    RobotSimGround & g;
    bool active = false;
    SimJointScalars sc{0, SIM_JOINT_DEFAULT_ACTIVATION, SIM_JOINT_DEFAULT_STOP_ERP};
    // the model, always [B][na] on the device; tau_max / damping / armature are handed to the kernel only if they were given
    double *tmax = nullptr, *dmp = nullptr, *arm = nullptr, *qlo = nullptr, *qhi = nullptr;
    bool have_tmax = false, have_dmp = false, have_arm = false;
    double * tau_applied = nullptr; // [B][na]
    int * rows = nullptr;           // [B][NJ]
    double * lams = nullptr;        // [B][NJ]
    int * dropped = nullptr;        // [B]
    // host-buffer form (n states, n need not be B): grown on demand
    int cap = 0;
    std::vector<void *> staging;
    double *hX = nullptr, *hTau = nullptr, *hV = nullptr, *hA = nullptr, *hLam = nullptr, *hLamC = nullptr, *hLam0 = nullptr, *hGap = nullptr, *hEnv = nullptr,
           *hRes = nullptr, *hModel = nullptr, *hTauA = nullptr, *hLamS = nullptr;
    unsigned * hCon = nullptr;
    int *hSw = nullptr, *hRows = nullptr, *hDrop = nullptr;

    // (nothing is allocated here: the host-buffer solve needs the staging only; the handle-owned arrays come with the first set_model)
    explicit RobotSimGroundJoint(RobotSimGround & ground) : g(ground) {}
    void allocate()
    {
      if (tau_applied != nullptr)
        return;
      RobotSimRt & sim = g.sim;
      const SimJointSizes z = sim_joint_sizes(sim.B, sim.sz.na);
      AllocScope scope; // (a failing allocation below releases the ones before it, and the pointers are kept only once all have succeeded)
      double * n_tmax = (double *)dev_alloc(z.array_bytes);
      double * n_dmp = (double *)dev_alloc(z.array_bytes);
      double * n_arm = (double *)dev_alloc(z.array_bytes);
      double * n_qlo = (double *)dev_alloc(z.array_bytes);
      double * n_qhi = (double *)dev_alloc(z.array_bytes);
      double * n_tau = (double *)dev_alloc(z.tau_bytes);
      int * n_rows = (int *)dev_alloc(z.rows_bytes);
      double * n_lams = (double *)dev_alloc(z.lam_bytes);
      int * n_dropped = (int *)dev_alloc(z.dropped_bytes);
      scope.commit();
      tmax = n_tmax;
      dmp = n_dmp;
      arm = n_arm;
      qlo = n_qlo;
      qhi = n_qhi;
      tau_applied = n_tau;
      rows = n_rows;
      lams = n_lams;
      dropped = n_dropped;
    }
    RobotSimGroundJoint(const RobotSimGroundJoint &) = delete;
    RobotSimGroundJoint & operator=(const RobotSimGroundJoint &) = delete;
    void zero_outputs()
    {
      RobotSimRt & sim = g.sim;
      const SimJointSizes z = sim_joint_sizes(sim.B, sim.sz.na);
      dev_zero(tau_applied, z.tau_bytes, sim.stream);
      dev_zero(rows, z.rows_bytes, sim.stream);
      dev_zero(lams, z.lam_bytes, sim.stream);
      dev_zero(dropped, z.dropped_bytes, sim.stream);
      stream_sync(sim.stream);
    }
    void free_staging()
    {
      for (void * p : staging)
        dev_free(p);
      staging.clear();
      hX = hTau = hV = hA = hLam = hLamC = hLam0 = hGap = hEnv = hRes = hModel = hTauA = hLamS = nullptr;
      hCon = nullptr;
      hSw = hRows = hDrop = nullptr;
      cap = 0;
    }
    ~RobotSimGroundJoint()
    {
      free_staging();
      dev_free(tmax);
      dev_free(dmp);
      dev_free(arm);
      dev_free(qlo);
      dev_free(qhi);
      dev_free(tau_applied);
      dev_free(rows);
      dev_free(lams);
      dev_free(dropped);
    }
    // (the caller has run sim_joint_admission_error) copies the model to the device, a row per robot, and zeroes the read-outs
    void set_model(const smpc_joint_model_settings * m, const double * tab_lo, const double * tab_hi)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const int B = sim.B, na = sim.sz.na;
      const size_t bytes = sim_joint_sizes(B, na).array_bytes;
      sim.wait(); // (a step in flight still reads the arrays that are replaced below)
      allocate();
      std::vector<double> h((size_t)B * na);
      auto put = [&](double * dst, const double * src, const double * fallback) {
        for (int i = 0; i < B; i++)
          for (int k = 0; k < na; k++)
            h[(size_t)i * na + k] = src ? src[(m->per_robot ? (size_t)i * na : (size_t)0) + k] : fallback[k];
        h2d(dst, h.data(), bytes, sim.stream);
        stream_sync(sim.stream); // (`h` is refilled for the next array)
      };
      if (m->tau_max)
        put(tmax, m->tau_max, nullptr);
      if (m->damping)
        put(dmp, m->damping, nullptr);
      if (m->armature)
        put(arm, m->armature, nullptr);
      put(qlo, m->q_lo, tab_lo);
      put(qhi, m->q_hi, tab_hi);
      have_tmax = m->tau_max != nullptr;
      have_dmp = m->damping != nullptr;
      have_arm = m->armature != nullptr;
      zero_outputs();
      sc = sim_joint_resolve(m);
      active = true;
    }
    // `terr` non-null: sim_ground_terrain_rt_body (a null `body` reads the table there); else `body` ([n][njoints][10] on the device)
    // non-null: sim_ground_body_rt_body, else the kernel of DESIGN 3.26
    // `pts` non-null: the body-point kernels of DESIGN 3.29, always at 32 rows, on the terrain or on the plane
    void run(int n, const SimGroundJointArgs & ja, const double * body = nullptr, const SimTerrainDev * terr = nullptr, const SimPointsDev * pts = nullptr)
    {
      if (pts != nullptr)
      {
        SimGroundPointsArgs pa;
        pa.t.b.j = ja;
        pa.t.b.body = body;
        pa.t.t = terr != nullptr ? *terr : SimTerrainDev{nullptr, nullptr, nullptr, 0, 0, 0, 0.0, nullptr, nullptr};
        pa.p = *pts;
        if (terr != nullptr)
          launch<SimGroundPointsArgs, sim_ground_points_terrain_rt_body<32>, 64, 1, 0>(n, g.sim.stream, pa);
        else
          launch<SimGroundPointsArgs, sim_ground_points_rt_body<32>, 64, 1, 0>(n, g.sim.stream, pa);
      }
      else if (terr != nullptr)
      {
        SimGroundTerrainArgs ta;
        ta.b.j = ja;
        ta.b.body = body;
        ta.t = *terr;
        if (g.gz.inst == 12)
          launch<SimGroundTerrainArgs, sim_ground_terrain_rt_body<24>, 64, 1, 0>(n, g.sim.stream, ta);
        else
          launch<SimGroundTerrainArgs, sim_ground_terrain_rt_body<32>, 64, 1, 0>(n, g.sim.stream, ta);
      }
      else if (body != nullptr)
      {
        SimGroundBodyArgs ba;
        ba.j = ja;
        ba.body = body;
        if (g.gz.inst == 12)
          launch<SimGroundBodyArgs, sim_ground_body_rt_body<24>, 64, 1, 0>(n, g.sim.stream, ba);
        else
          launch<SimGroundBodyArgs, sim_ground_body_rt_body<32>, 64, 1, 0>(n, g.sim.stream, ba);
      }
      else if (g.gz.inst == 12)
        launch<SimGroundJointArgs, sim_ground_joint_rt_body<24>, 64, 1, 0>(n, g.sim.stream, ja);
      else
        launch<SimGroundJointArgs, sim_ground_joint_rt_body<32>, 64, 1, 0>(n, g.sim.stream, ja);
    }
    // `env` and `ws` may be null or inactive: the handle's uniform ground, no push; `sweeps` sweeps from zero.  Before set_model every
    // array is null and stops = 0: the inert model (a handle with body parameters and no joint model steps through here).
    void step_device(double * X_dev, const double * tau_dev, double dt, const RobotSimGroundEnv * env, RobotSimGroundWs * ws, const double * body = nullptr,
                     const SimTerrainDev * terr = nullptr, const SimPointsDev * pts = nullptr)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      SimGroundJointArgs ja;
      SimGroundWsArgs & wa = ja.w;
      wa.e.g = g.args(dt);
      wa.e.g.X = X_dev;
      wa.e.g.tau = tau_dev;
      wa.e.g.advance = 1;
      wa.e.g.a_out = sim.a;
      wa.e.g.lam_out = g.lam;
      wa.e.g.contact_out = g.contact;
      const bool have = env != nullptr && env->active;
      wa.e.plane = have ? env->plane : nullptr;
      wa.e.mu = have ? env->mu : nullptr;
      wa.e.push = have ? env->push : nullptr;
      wa.e.push_joint = have ? env->push_joint : 0;
      const bool solver = ws != nullptr && ws->active;
      wa.lam0 = solver ? ws->warm : nullptr;
      wa.lamc_out = solver ? ws->warm : nullptr;
      wa.sweeps_out = solver ? ws->sweeps : nullptr;
      wa.resid_out = solver ? ws->resid : nullptr;
      wa.warm_start = solver ? ws->ws.warm_start : 0;
      wa.min_sweeps = solver ? ws->ws.min_sweeps : 1;
      wa.tol = solver ? ws->ws.tol : 0.0;
      ja.tau_max = have_tmax ? tmax : nullptr;
      ja.damping = have_dmp ? dmp : nullptr;
      ja.armature = have_arm ? arm : nullptr;
      ja.q_lo = qlo;
      ja.q_hi = qhi;
      ja.per_robot = 1;
      ja.stops = sc.stops;
      ja.activation = sc.activation;
      ja.stop_erp = sc.stop_erp;
      ja.tau_out = tau_applied;
      ja.rows_out = rows;
      ja.lams_out = lams;
      ja.dropped_out = dropped;
      run(sim.B, ja, body, terr, pts);
    }
    void read_last(double * tau_out, int * rows_out, double * lams_out, int * dropped_out)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const SimJointSizes z = sim_joint_sizes(sim.B, sim.sz.na);
      if (tau_out)
        d2h(tau_out, tau_applied, z.tau_bytes, sim.stream);
      if (rows_out)
        d2h(rows_out, rows, z.rows_bytes, sim.stream);
      if (lams_out)
        d2h(lams_out, lams, z.lam_bytes, sim.stream);
      if (dropped_out)
        d2h(dropped_out, dropped, z.dropped_bytes, sim.stream);
      stream_sync(sim.stream);
    }
    template <class T>
    T * stage(size_t count)
    {
      staging.push_back(nullptr); // (the slot first: a failing push_back after the allocation would lose the pointer)
      T * p = (T *)dev_alloc(count * sizeof(T));
      staging.back() = p;
      return p;
    }
    // (the caller has run the admissions) `m` may be null: the inert model; `body_dev` ([n][njoints][10], device, complete on the stream) or null
    void dynamics(int n, const double * X, const double * tau, double dt, const double * plane_h, const double * mu_h, const double * push_h, int joint,
                  const SimGroundWsSettings & st, const double * lam0_h, const smpc_joint_model_settings * m, const double * tab_lo, const double * tab_hi,
                  double * v_out, double * a_out, double * lam_out, double * lamc_out, double * gap_out, unsigned * con_out, int * sweeps_out, double * resid_out,
                  double * tau_applied_out, int * rows_out, double * lams_out, int * dropped_out, const double * body_dev = nullptr,
                  const SimTerrainDev * terr = nullptr, const SimPointsDev * pts = nullptr)
    {
      if (n < 1)
        throw InvalidCall("n must be positive");
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const SimRtSizes & sz = sim.sz;
      const SimGroundSizes & gz = g.gz;
      stream_t stream = sim.stream;
      constexpr int NE = SIM_GROUND_ENV_DOUBLES, NJ = SIM_JOINT_MAX_STOPS;
      const int na = sz.na;
      if (n > cap)
      {
        stream_sync(stream);
        free_staging();
        try
        {
          hX = stage<double>((size_t)n * sz.nx);
          hTau = stage<double>((size_t)n * na);
          hV = stage<double>((size_t)n * sz.nv);
          hA = stage<double>((size_t)n * sz.nv);
          hLam = stage<double>((size_t)n * gz.nrows);
          hLamC = stage<double>((size_t)n * gz.nrows);
          hLam0 = stage<double>((size_t)n * gz.nrows);
          hGap = stage<double>((size_t)n * gz.npts);
          hEnv = stage<double>((size_t)n * NE); // planes [n][4] | mu [n] | pushes [n][6]
          hRes = stage<double>((size_t)n);
          hModel = stage<double>((size_t)5 * n * na); // tau_max | damping | armature | q_lo | q_hi, [n][na] each
          hTauA = stage<double>((size_t)n * na);
          hLamS = stage<double>((size_t)n * NJ);
          hCon = stage<unsigned>((size_t)n);
          hSw = stage<int>((size_t)n);
          hRows = stage<int>((size_t)n * NJ);
          hDrop = stage<int>((size_t)n);
        }
        catch (...)
        {
          free_staging();
          throw;
        }
        cap = n;
      }
      double *dPlane = hEnv, *dMu = hEnv + (size_t)cap * 4, *dPush = hEnv + (size_t)cap * 5;
      h2d(hX, X, (size_t)n * sz.nx * sizeof(double), stream);
      h2d(hTau, tau, (size_t)n * na * sizeof(double), stream);
      if (plane_h)
        h2d(dPlane, plane_h, (size_t)n * 4 * sizeof(double), stream);
      if (mu_h)
        h2d(dMu, mu_h, (size_t)n * sizeof(double), stream);
      if (push_h)
        h2d(dPush, push_h, (size_t)n * 6 * sizeof(double), stream);
      const bool start = st.warm_start != 0 && lam0_h != nullptr;
      if (start)
        h2d(hLam0, lam0_h, (size_t)n * gz.nrows * sizeof(double), stream);
      const int per_robot = m && m->per_robot ? 1 : 0;
      const size_t count = (size_t)(per_robot ? n : 1) * na;
      const double * src[5] = {m ? m->tau_max : nullptr, m ? m->damping : nullptr, m ? m->armature : nullptr, m && m->q_lo ? m->q_lo : tab_lo,
                               m && m->q_hi ? m->q_hi : tab_hi};
      // (a table row beside per-robot rows: every array of a launch has one stride, so the table's limits are repeated per robot)
      std::vector<double> rep;
      const double * dev[5];
      for (int a = 0; a < 5; a++)
      {
        double * dst = hModel + (size_t)a * cap * na;
        dev[a] = src[a] ? dst : nullptr;
        if (!src[a])
          continue;
        const bool table = a >= 3 && !(m && (a == 3 ? m->q_lo : m->q_hi));
        if (table && per_robot)
        {
          rep.resize((size_t)n * na);
          for (int i = 0; i < n; i++)
            for (int k = 0; k < na; k++)
              rep[(size_t)i * na + k] = src[a][k];
          h2d(dst, rep.data(), rep.size() * sizeof(double), stream);
          stream_sync(stream); // (`rep` is refilled for the next array)
        }
        else
          h2d(dst, src[a], count * sizeof(double), stream);
      }
      const SimJointScalars js = sim_joint_resolve(m);
      SimGroundJointArgs ja;
      SimGroundWsArgs & wa = ja.w;
      wa.e.g = g.args(dt);
      wa.e.g.X = hX;
      wa.e.g.tau = hTau;
      wa.e.g.advance = 0;
      wa.e.g.a_out = hA;
      wa.e.g.lam_out = hLam;
      wa.e.g.contact_out = hCon;
      wa.e.g.vnext_out = hV;
      wa.e.g.gap_out = hGap;
      wa.e.plane = plane_h ? dPlane : nullptr;
      wa.e.mu = mu_h ? dMu : nullptr;
      wa.e.push = push_h ? dPush : nullptr;
      wa.e.push_joint = joint;
      wa.lam0 = start ? hLam0 : nullptr;
      wa.lamc_out = hLamC;
      wa.sweeps_out = hSw;
      wa.resid_out = hRes;
      wa.warm_start = start ? 1 : 0;
      wa.min_sweeps = st.min_sweeps;
      wa.tol = st.tol;
      ja.tau_max = dev[0];
      ja.damping = dev[1];
      ja.armature = dev[2];
      ja.q_lo = dev[3];
      ja.q_hi = dev[4];
      ja.per_robot = per_robot;
      ja.stops = js.stops;
      ja.activation = js.activation;
      ja.stop_erp = js.stop_erp;
      ja.tau_out = hTauA;
      ja.rows_out = hRows;
      ja.lams_out = hLamS;
      ja.dropped_out = hDrop;
      run(n, ja, body_dev, terr, pts);
      if (v_out)
        d2h(v_out, hV, (size_t)n * sz.nv * sizeof(double), stream);
      if (a_out)
        d2h(a_out, hA, (size_t)n * sz.nv * sizeof(double), stream);
      if (lam_out)
        d2h(lam_out, hLam, (size_t)n * gz.nrows * sizeof(double), stream);
      if (lamc_out)
        d2h(lamc_out, hLamC, (size_t)n * gz.nrows * sizeof(double), stream);
      if (gap_out)
        d2h(gap_out, hGap, (size_t)n * gz.npts * sizeof(double), stream);
      if (con_out)
        d2h(con_out, hCon, (size_t)n * sizeof(unsigned), stream);
      if (sweeps_out)
        d2h(sweeps_out, hSw, (size_t)n * sizeof(int), stream);
      if (resid_out)
        d2h(resid_out, hRes, (size_t)n * sizeof(double), stream);
      if (tau_applied_out)
        d2h(tau_applied_out, hTauA, (size_t)n * na * sizeof(double), stream);
      if (rows_out)
        d2h(rows_out, hRows, (size_t)n * NJ * sizeof(int), stream);
      if (lams_out)
        d2h(lams_out, hLamS, (size_t)n * NJ * sizeof(double), stream);
      if (dropped_out)
        d2h(dropped_out, hDrop, (size_t)n * sizeof(int), stream);
      stream_sync(stream);
    }
  };

  // ---- host: the per-robot body parameters of one simulator handle's ground (a sibling of RobotSimGroundJoint, whose
  // step_device and dynamics take the device pointers handed out here).  `active` between set(rows) and set(null): while it is, the
  // handle's ground steps launch sim_ground_body_rt_body.  The staging of the host-buffer solve never touches the handle's own array. ----
  struct RobotSimGroundBody
  {
    RobotSimGround & g;
    bool active = false;
    double * body = nullptr;  // [B][njoints][10], kept once allocated (the pointer handed out stays valid across set calls)
    double * hBody = nullptr; // host-buffer form: [cap][njoints][10], grown on demand
    int cap = 0;

    explicit RobotSimGroundBody(RobotSimGround & ground) : g(ground) {}
    RobotSimGroundBody(const RobotSimGroundBody &) = delete;
    RobotSimGroundBody & operator=(const RobotSimGroundBody &) = delete;
    ~RobotSimGroundBody()
    {
      dev_free(body);
      dev_free(hBody);
    }
    int njoints() const { return g.sim.sz.nq - 6; }
    // (the caller has run sim_body_admission_error) rows [B][njoints][10] to the device; null clears: the handle launches what it launched before
    void set(const double * rows)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      sim.wait(); // (a step in flight still reads the array)
      if (!rows)
      {
        active = false;
        return;
      }
      const size_t bytes = sim_body_bytes(sim.B, njoints());
      if (!body)
        body = (double *)dev_alloc(bytes);
      h2d(body, rows, bytes, sim.stream);
      stream_sync(sim.stream);
      active = true;
    }
    void read(double * out)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      d2h(out, body, sim_body_bytes(sim.B, njoints()), sim.stream);
      stream_sync(sim.stream);
    }
    // rows [n][njoints][10] of a host-buffer solve to the staging array, on the handle's stream; the device pointer for RobotSimGroundJoint::dynamics
    const double * stage(int n, const double * rows)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      if (n > cap)
      {
        stream_sync(sim.stream);
        dev_free(hBody);
        hBody = nullptr;
        cap = 0;
        hBody = (double *)dev_alloc(sim_body_bytes(n, njoints()));
        cap = n;
      }
      h2d(hBody, rows, sim_body_bytes(n, njoints()), sim.stream);
      return hBody;
    }
  };

  // ---- host: the per-robot height-field terrain of one simulator handle's ground (a sibling of RobotSimGroundBody, whose
  // device view RobotSimGroundJoint::step_device and dynamics take).  `active` between set(settings) and set(null): while it is, the
  // handle's ground steps launch sim_ground_terrain_rt_body.  The staging of the host-buffer solve never touches the handle's own arrays. ----
  struct RobotSimGroundTerrain
  {
    RobotSimGround & g;
    bool active = false;
    int nx = 0, ny = 0, tiles = 0;
    double cell = 0.0;
    double * heights = nullptr; // [tiles][ny][nx]
    int * tile = nullptr;       // [B]
    double * origin = nullptr;  // [B][2]
    double * n_last = nullptr;  // [B][points][3]
    double * h_last = nullptr;  // [B][points]
    // host-buffer form (n states): grown on demand
    int cap = 0;
    size_t hcap = 0;
    double *sHeights = nullptr, *sOrigin = nullptr, *sN = nullptr, *sH = nullptr;
    int * sTile = nullptr;

    explicit RobotSimGroundTerrain(RobotSimGround & ground) : g(ground) {}
    RobotSimGroundTerrain(const RobotSimGroundTerrain &) = delete;
    RobotSimGroundTerrain & operator=(const RobotSimGroundTerrain &) = delete;
    void free_staging()
    {
      dev_free(sHeights);
      dev_free(sOrigin);
      dev_free(sN);
      dev_free(sH);
      dev_free(sTile);
      sHeights = sOrigin = sN = sH = nullptr;
      sTile = nullptr;
      cap = 0;
      hcap = 0;
    }
    ~RobotSimGroundTerrain()
    {
      free_staging();
      dev_free(heights);
      dev_free(tile);
      dev_free(origin);
      dev_free(n_last);
      dev_free(h_last);
    }
    // (the caller has run sim_terrain_admission_error) the settings to the device; null clears: the handle launches what it launched before
    void set(const smpc_terrain_settings * t)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      sim.wait(); // (a step in flight still reads the arrays)
      if (!t)
      {
        active = false;
        return;
      }
      const int B = sim.B, npts = g.gz.npts;
      const size_t hb = sim_terrain_height_bytes(t->tiles, t->ny, t->nx);
      {
        AllocScope scope; // (a failing allocation releases the ones before it; the old arrays stay until all have succeeded)
        double * n_heights = (double *)dev_alloc(hb);
        int * n_tile = tile ? nullptr : (int *)dev_alloc(sim_terrain_tile_bytes(B));
        double * n_origin = origin ? nullptr : (double *)dev_alloc(sim_terrain_origin_bytes(B));
        double * n_n = n_last ? nullptr : (double *)dev_alloc(sim_terrain_normal_bytes(B, npts));
        double * n_h = h_last ? nullptr : (double *)dev_alloc(sim_terrain_hlast_bytes(B, npts));
        scope.commit();
        dev_free(heights);
        heights = n_heights;
        if (n_tile)
          tile = n_tile;
        if (n_origin)
          origin = n_origin;
        if (n_n)
          n_last = n_n;
        if (n_h)
          h_last = n_h;
      }
      std::vector<int> ht((size_t)B, 0);
      std::vector<double> ho((size_t)B * 2, 0.0);
      if (t->tile)
        ht.assign(t->tile, t->tile + B);
      if (t->origin)
        ho.assign(t->origin, t->origin + (size_t)B * 2);
      h2d(heights, t->heights, hb, sim.stream);
      h2d(tile, ht.data(), sim_terrain_tile_bytes(B), sim.stream);
      h2d(origin, ho.data(), sim_terrain_origin_bytes(B), sim.stream);
      dev_zero(n_last, sim_terrain_normal_bytes(B, npts), sim.stream);
      dev_zero(h_last, sim_terrain_hlast_bytes(B, npts), sim.stream);
      stream_sync(sim.stream);
      nx = t->nx;
      ny = t->ny;
      tiles = t->tiles;
      cell = t->cell;
      active = true;
    }
    // the device view of the handle's terrain for a step
    SimTerrainDev view() const
    {
      SimTerrainDev d;
      d.heights = heights;
      d.tile = tile;
      d.origin = origin;
      d.nx = nx;
      d.ny = ny;
      d.tiles = tiles;
      d.cell = cell;
      d.n_out = n_last;
      d.h_out = h_last;
      return d;
    }
    void read_last(double * normals_out, double * heights_out)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      if (normals_out)
        d2h(normals_out, n_last, sim_terrain_normal_bytes(sim.B, g.gz.npts), sim.stream);
      if (heights_out)
        d2h(heights_out, h_last, sim_terrain_hlast_bytes(sim.B, g.gz.npts), sim.stream);
      stream_sync(sim.stream);
    }
    // the settings of a host-buffer solve of n states to the staging arrays, on the handle's stream; the device view for RobotSimGroundJoint::dynamics
    SimTerrainDev stage(int n, const smpc_terrain_settings * t)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      const int npts = g.gz.npts;
      const size_t hb = sim_terrain_height_bytes(t->tiles, t->ny, t->nx);
      if (n > cap || hb > hcap)
      {
        stream_sync(sim.stream);
        const int ncap = n > cap ? n : cap;
        const size_t nh = hb > hcap ? hb : hcap;
        free_staging();
        try
        {
          sHeights = (double *)dev_alloc(nh);
          sTile = (int *)dev_alloc(sim_terrain_tile_bytes(ncap));
          sOrigin = (double *)dev_alloc(sim_terrain_origin_bytes(ncap));
          sN = (double *)dev_alloc(sim_terrain_normal_bytes(ncap, npts));
          sH = (double *)dev_alloc(sim_terrain_hlast_bytes(ncap, npts));
        }
        catch (...)
        {
          free_staging();
          throw;
        }
        cap = ncap;
        hcap = nh;
      }
      h2d(sHeights, t->heights, hb, sim.stream);
      if (t->tile)
        h2d(sTile, t->tile, sim_terrain_tile_bytes(n), sim.stream);
      if (t->origin)
        h2d(sOrigin, t->origin, sim_terrain_origin_bytes(n), sim.stream);
      SimTerrainDev d;
      d.heights = sHeights;
      d.tile = t->tile ? sTile : nullptr;
      d.origin = t->origin ? sOrigin : nullptr;
      d.nx = t->nx;
      d.ny = t->ny;
      d.tiles = t->tiles;
      d.cell = t->cell;
      d.n_out = sN;
      d.h_out = sH;
      return d;
    }
    // (after the solve) the two read-outs of the staging arrays
    void read_staged(int n, double * normals_out, double * heights_out)
    {
      RobotSimRt & sim = g.sim;
      if (normals_out)
        d2h(normals_out, sN, sim_terrain_normal_bytes(n, g.gz.npts), sim.stream);
      if (heights_out)
        d2h(heights_out, sH, sim_terrain_hlast_bytes(n, g.gz.npts), sim.stream);
      stream_sync(sim.stream);
    }
  };

  // ---- host: the body points of one simulator handle's ground (a sibling of RobotSimGroundTerrain, whose device view
  // RobotSimGroundJoint::step_device and dynamics take).  `active` between set(settings with n > 0) and set(null or n = 0): while it is,
  // the handle's ground steps launch a body-point kernel.  The staging of the host-buffer solve never touches the handle's own arrays. ----
  struct RobotSimGroundPoints
  {
    struct Arrays
    {
      int * joint = nullptr;             // [16]
      double * offset = nullptr;         // [16][3]
      int * slots = nullptr;             // [n][8]
      double * lam = nullptr;            // [n][8][3]
      double * gap = nullptr;            // [n][16]
      int * dropped = nullptr;           // [n]
      unsigned char * touch = nullptr;   // [n]
      void release()
      {
        dev_free(joint);
        dev_free(offset);
        dev_free(slots);
        dev_free(lam);
        dev_free(gap);
        dev_free(dropped);
        dev_free(touch);
        *this = Arrays();
      }
    };
    RobotSimGround & g;
    bool active = false;
    int n = 0;
    double band = SIM_POINTS_DEFAULT_BAND;
    Arrays own; // the handle's points and the read-outs of its last step, [B]
    Arrays st;  // host-buffer form: [cap], grown on demand
    int cap = 0;

    explicit RobotSimGroundPoints(RobotSimGround & ground) : g(ground) {}
    RobotSimGroundPoints(const RobotSimGroundPoints &) = delete;
    RobotSimGroundPoints & operator=(const RobotSimGroundPoints &) = delete;
    ~RobotSimGroundPoints()
    {
      own.release();
      st.release();
    }
    static void allocate(Arrays & a, int count)
    {
      AllocScope scope; // (a failing allocation releases the ones before it; the pointers are kept only once all have succeeded)
      Arrays t;
      t.joint = (int *)dev_alloc(sim_points_joint_bytes());
      t.offset = (double *)dev_alloc(sim_points_offset_bytes());
      t.slots = (int *)dev_alloc(sim_points_slots_bytes(count));
      t.lam = (double *)dev_alloc(sim_points_lam_bytes(count));
      t.gap = (double *)dev_alloc(sim_points_gap_bytes(count));
      t.dropped = (int *)dev_alloc(sim_points_dropped_bytes(count));
      t.touch = (unsigned char *)dev_alloc(sim_points_touch_bytes(count));
      scope.commit();
      a = t;
    }
    static void upload(const Arrays & a, const smpc_body_points_settings * s, stream_t stream)
    {
      int hj[SIM_POINTS_MAX];
      double ho[SIM_POINTS_MAX * 3];
      for (int k = 0; k < SIM_POINTS_MAX; k++)
      {
        hj[k] = k < s->n ? s->joint[k] : 0;
        for (int i = 0; i < 3; i++)
          ho[k * 3 + i] = k < s->n ? s->offset[k][i] : 0.0;
      }
      h2d(a.joint, hj, sizeof(hj), stream);
      h2d(a.offset, ho, sizeof(ho), stream);
      stream_sync(stream); // (the two host arrays leave scope)
    }
    static SimPointsDev view_of(const Arrays & a, int n, double band)
    {
      SimPointsDev d;
      d.joint = a.joint;
      d.offset = a.offset;
      d.n = n;
      d.band = band;
      d.slots_out = a.slots;
      d.lam_out = a.lam;
      d.gap_out = a.gap;
      d.dropped_out = a.dropped;
      d.touch_out = a.touch;
      return d;
    }
    void zero(const Arrays & a, int count)
    {
      stream_t stream = g.sim.stream;
      dev_zero(a.slots, sim_points_slots_bytes(count), stream);
      dev_zero(a.lam, sim_points_lam_bytes(count), stream);
      dev_zero(a.gap, sim_points_gap_bytes(count), stream);
      dev_zero(a.dropped, sim_points_dropped_bytes(count), stream);
      dev_zero(a.touch, sim_points_touch_bytes(count), stream);
    }
    // (the caller has run sim_points_admission_error) the settings to the device; null or n = 0 clears: the handle launches what it launched before
    void set(const smpc_body_points_settings * s)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      sim.wait(); // (a step in flight still reads the arrays)
      if (!s || s->n == 0)
      {
        active = false;
        return;
      }
      if (!own.joint)
        allocate(own, sim.B);
      upload(own, s, sim.stream);
      zero(own, sim.B);
      stream_sync(sim.stream);
      n = s->n;
      band = sim_points_band(s->band);
      active = true;
    }
    // the device view of the handle's points for a step
    SimPointsDev view() const { return view_of(own, n, band); }
    static void read_from(const Arrays & a, int count, stream_t stream, int * slots_out, double * lam_out, double * gap_out, int * dropped_out,
                          unsigned char * touch_out)
    {
      if (slots_out)
        d2h(slots_out, a.slots, sim_points_slots_bytes(count), stream);
      if (lam_out)
        d2h(lam_out, a.lam, sim_points_lam_bytes(count), stream);
      if (gap_out)
        d2h(gap_out, a.gap, sim_points_gap_bytes(count), stream);
      if (dropped_out)
        d2h(dropped_out, a.dropped, sim_points_dropped_bytes(count), stream);
      if (touch_out)
        d2h(touch_out, a.touch, sim_points_touch_bytes(count), stream);
      stream_sync(stream);
    }
    void read_last(int * slots_out, double * lam_out, double * gap_out, int * dropped_out, unsigned char * touch_out)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      read_from(own, sim.B, sim.stream, slots_out, lam_out, gap_out, dropped_out, touch_out);
    }
    // the settings of a host-buffer solve of `count` states (s->n > 0) to the staging arrays, on the handle's stream; the device view for
    // RobotSimGroundJoint::dynamics
    SimPointsDev stage(int count, const smpc_body_points_settings * s)
    {
      RobotSimRt & sim = g.sim;
      set_device(sim.device_id);
      if (count > cap)
      {
        stream_sync(sim.stream);
        st.release();
        cap = 0;
        allocate(st, count);
        cap = count;
      }
      upload(st, s, sim.stream);
      return view_of(st, s->n, sim_points_band(s->band));
    }
    // (after the solve) the five read-outs of the staging arrays
    void read_staged(int count, int * slots_out, double * lam_out, double * gap_out, int * dropped_out, unsigned char * touch_out)
    {
      read_from(st, count, g.sim.stream, slots_out, lam_out, gap_out, dropped_out, touch_out);
    }
  };
} // namespace smpc
