// The terrain of the C++ host mirror (include/simple-mpc/batched-sim.hpp: setTerrain, clearTerrain, terrainDevicePointers,
// lastTerrainNormals, lastTerrainHeights, groundTerrainDynamics, terrain_height, terrain_from_function) on the built-in quadruped: the
// mirror against the C ABI called directly, bit for bit, in the host-buffer solve and over 30 steps on a rough tile; a flat tile against the
// kernels on the plane bit for bit; the recorded normals and heights against terrain_height at the contact points' tile; clearing, setGround
// and the refusals.  "Device" memory: plain host memory for the sequential-lane test build, hipMalloc'ed memory for the HIP library
// (SMPC_CHECK_HIP).
#include "simple-mpc/batched-sim.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#ifdef SMPC_CHECK_HIP
#include <hip/hip_runtime.h>
#endif

#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);                                                      \
      return 1;                                                                                                        \
    }                                                                                                                  \
  } while (0)

template <class F>
static std::string refusal(F && f)
{
  try
  {
    f();
  }
  catch (const std::runtime_error & e)
  {
    return e.what();
  }
  return std::string();
}

// a buffer the simulator's stream can reach
struct DeviceBuffer
{
  double * p = nullptr;
  size_t n;
  explicit DeviceBuffer(const std::vector<double> & v) : n(v.size())
  {
#ifdef SMPC_CHECK_HIP
    if (hipMalloc((void **)&p, n * sizeof(double)) != hipSuccess || hipMemcpy(p, v.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      throw std::runtime_error("device buffer");
#else
    p = new double[n];
    std::memcpy(p, v.data(), n * sizeof(double));
#endif
  }
  std::vector<double> get() const
  {
    std::vector<double> v(n);
#ifdef SMPC_CHECK_HIP
    if (hipMemcpy(v.data(), p, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      throw std::runtime_error("device buffer");
#else
    std::memcpy(v.data(), p, n * sizeof(double));
#endif
    return v;
  }
  ~DeviceBuffer()
  {
#ifdef SMPC_CHECK_HIP
    (void)hipFree(p);
#else
    delete[] p;
#endif
  }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer & operator=(const DeviceBuffer &) = delete;
};

int main()
{
  const smpc_robot_model * robot = smpc_builtin_robot("go2_like");
  CHECK(robot != nullptr);
  const int B = 3, NJ = SMPC_JOINT_MAX_STOPS, steps = 30;
  const double dt = 1e-3;
  typedef simple_mpc::BatchedRobotSim Sim;
  typedef Sim::JointModel JM;
  typedef Sim::GroundJoint GJ;
  typedef Sim::GroundTerrain GT;
  Sim sim(robot, 3, B), twin(robot, 3, B), plain(robot, 3, B);
  const int nq = sim.nq(), nv = sim.nv(), nx = nq + nv, na = nv - 6;
  std::vector<double> X((size_t)B * nx, 0.0), tau((size_t)B * na, 0.0);
  for (int i = 0; i < B; i++)
  {
    for (int k = 0; k < nq; k++)
      X[(size_t)i * nx + k] = robot->q_ref[k];
    X[(size_t)i * nx + nq + 2] = -0.2 - 0.1 * i; // (moving down onto the ground)
    for (int k = 0; k < na; k++)
      tau[(size_t)i * na + k] = (k % 2 ? -1.0 : 1.0) * (0.5 + 0.1 * k + 0.3 * i);
  }
  const double gz = robot->q_ref[2] + robot->foot_ref_p[0][2] + 0.002; // (the feet of the reference pose 2 mm inside the flat ground)
  // ---- the helpers: a tile from a function, and the sampling ----
  const int TNX = 9, TNY = 7;
  const double cell = 0.15;
  const std::vector<double> wavy =
      simple_mpc::terrain_from_function([&](double x, double y) { return gz + 0.02 * std::sin(7.0 * x) * std::cos(5.0 * y); }, TNX, TNY, cell);
  CHECK((int)wavy.size() == TNX * TNY && wavy[(size_t)2 * TNX + 3] == gz + 0.02 * std::sin(7.0 * 3 * cell) * std::cos(5.0 * 2 * cell));
  CHECK(refusal([&] { simple_mpc::terrain_from_function([](double, double) { return 0.0; }, 1, 4, 0.1); }).find("terrain_from_function") != std::string::npos);
  {
    const std::vector<double> tilt = simple_mpc::terrain_from_function([](double x, double y) { return 0.1 * x - 0.2 * y; }, 6, 4, 0.25);
    const simple_mpc::TerrainSample s = simple_mpc::terrain_height(tilt, 6, 4, 0.25, 1.0, -1.0, 1.4, -0.7);
    const double q = 1.0 / std::sqrt(1.05);
    CHECK(std::fabs(s.h - (0.04 - 0.06)) < 1e-15 && std::fabs(s.n[0] + 0.1 * q) < 1e-15 && std::fabs(s.n[1] - 0.2 * q) < 1e-15 && std::fabs(s.n[2] - q) < 1e-15);
    const simple_mpc::TerrainSample f = simple_mpc::terrain_height(std::vector<double>(4, 0.37), 2, 2, 0.5, 0.0, 0.0, NAN, -INFINITY);
    CHECK(f.h == 0.37 && f.n[0] == 0.0 && f.n[1] == 0.0 && f.n[2] == 1.0);
    const simple_mpc::TerrainSample o = simple_mpc::terrain_height(tilt, 6, 4, 0.25, 0.0, 0.0, 1e300, -1e300); // clamped to the last / first node
    CHECK(std::fabs(o.h - 0.125) < 1e-15);
    CHECK(refusal([&] { simple_mpc::terrain_height(tilt, 6, 5, 0.25, 0.0, 0.0, 0.0, 0.0); }).find("terrain_height") != std::string::npos);
  }
  Sim::Terrain rough;
  rough.nx = TNX;
  rough.ny = TNY;
  rough.tiles = 2;
  rough.cell = cell;
  rough.heights = wavy;
  for (size_t k = 0; k < wavy.size(); k++)
    rough.heights.push_back(gz + (wavy[k] - gz) * 0.5); // (tile 1: half the amplitude)
  rough.tile = {0, 1, 0};
  for (int i = 0; i < B; i++)
  {
    rough.origin.push_back(robot->q_ref[0] - 0.6 + 0.03 * i);
    rough.origin.push_back(robot->q_ref[1] - 0.45 - 0.02 * i);
  }
  Sim::Terrain flat;
  flat.nx = 3;
  flat.ny = 2;
  flat.cell = 0.4;
  flat.heights.assign(6, gz);
  // before setGround
  CHECK(refusal([&] { sim.setTerrain(rough); }).find("smpc_robot_sim_set_ground") != std::string::npos);
  CHECK(sim.terrainDevicePointers().heights == nullptr);
  smpc_ground_settings gs;
  std::memset(&gs, 0, sizeof(gs));
  gs.ground_z = gz;
  sim.setGround(gs);
  twin.setGround(gs);
  plain.setGround(gs);
  sim.clearTerrain(); // (nothing to clear)
  CHECK(sim.terrainDevicePointers().heights == nullptr && sim.terrainDevicePointers().nx == 0);
  JM model;
  model.damping.assign(na, 0.1);
  model.tau_max.assign((size_t)B * na, 20.0);
  model.stops = true;
  // ---- the host-buffer solve: the mirror against the C ABI, bit for bit; a flat tile against groundJointDynamics on the plane ----
  {
    const GT r = sim.groundTerrainDynamics(X, tau, dt, rough, model);
    std::vector<double> dmp((size_t)B * na, 0.1);
    const smpc_joint_model_settings m = {model.tau_max.data(), dmp.data(), nullptr, nullptr, nullptr, 1, 1, 0.0, 0.0};
    const smpc_terrain_settings t = {TNX, TNY, 2, cell, rough.heights.data(), rough.tile.data(), rough.origin.data()};
    std::vector<double> v((size_t)B * nv), a((size_t)B * nv), lam((size_t)B * 12), lamc((size_t)B * 12), gap((size_t)B * 4), res(B), ta((size_t)B * na),
        ls((size_t)B * NJ), nrm((size_t)B * 12), hts((size_t)B * 4);
    std::vector<uint32_t> con(B);
    std::vector<int32_t> sw(B), rows((size_t)B * NJ), dr(B);
    CHECK(smpc_robot_sim_ground_terrain_dynamics(sim.handle(), B, X.data(), tau.data(), dt, &t, nullptr, nullptr, 0, nullptr, nullptr, &m, nullptr, v.data(), a.data(),
                                                 lam.data(), lamc.data(), gap.data(), con.data(), sw.data(), res.data(), ta.data(), rows.data(), ls.data(), dr.data(),
                                                 nrm.data(), hts.data()) == 0);
    const GJ & j = r.j;
    CHECK(j.s.g.v_next == v && j.s.g.a == a && j.s.g.lambda == lam && j.s.lambda_contact == lamc && j.s.g.gap == gap && j.s.g.contact == con);
    CHECK(j.s.sweeps == sw && j.s.residual == res && j.tau_applied == ta && j.stops.stop_rows == rows && j.stops.lam_stop == ls && j.stops.dropped == dr);
    CHECK(r.normals == nrm && r.heights == hts);
    CHECK(con[0] != 0 && con[1] != 0 && con[2] != 0);
    // the recorded heights and normals are terrain_height at a point whose gap says where it is: gap = n.z (p.z - h)
    double tilted = 0.0;
    for (int i = 0; i < B; i++)
      for (int c = 0; c < 4; c++)
      {
        const double * n = &nrm[((size_t)i * 4 + c) * 3];
        CHECK(std::fabs(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] - 1.0) < 1e-14 && n[2] > 0.5);
        CHECK(std::fabs(hts[(size_t)i * 4 + c] - gz) <= (rough.tile[i] == 0 ? 0.02 : 0.01) + 1e-15);
        tilted = std::fmax(tilted, std::fabs(n[0]));
      }
    CHECK(tilted > 0.01);
    const GJ q = sim.groundJointDynamics(X, tau, dt, model);
    const GT e = sim.groundTerrainDynamics(X, tau, dt, flat, model);
    CHECK(q.s.g.v_next == e.j.s.g.v_next && q.s.g.a == e.j.s.g.a && q.s.g.lambda == e.j.s.g.lambda && q.s.g.gap == e.j.s.g.gap && q.s.sweeps == e.j.s.sweeps);
    CHECK(q.s.residual == e.j.s.residual && q.tau_applied == e.j.tau_applied && q.s.lambda_contact == e.j.s.lambda_contact);
    CHECK(e.heights == std::vector<double>((size_t)B * 4, gz));
    CHECK(!(q.s.g.a == j.s.g.a));
    // one state of the three: n need not be the batch
    const std::vector<double> X1(X.begin() + nx, X.begin() + 2 * nx), t1(tau.begin() + na, tau.begin() + 2 * na);
    JM one = model;
    one.tau_max.assign(na, 20.0);
    Sim::Terrain r1 = rough;
    r1.tile = {rough.tile[1]};
    r1.origin = {rough.origin[2], rough.origin[3]};
    const GT s = sim.groundTerrainDynamics(X1, t1, dt, r1, one);
    CHECK(std::vector<double>(a.begin() + nv, a.begin() + 2 * nv) == s.j.s.g.a && std::vector<double>(lam.begin() + 12, lam.begin() + 24) == s.j.s.g.lambda);
    CHECK(std::vector<double>(nrm.begin() + 12, nrm.begin() + 24) == s.normals && std::vector<double>(hts.begin() + 4, hts.begin() + 8) == s.heights);
  }
  // ---- 30 steps: setTerrain of the mirror against smpc_robot_sim_set_terrain called directly; a flat tile against no terrain ----
  sim.setTerrain(rough);
  {
    const smpc_terrain_settings t = {TNX, TNY, 2, cell, rough.heights.data(), rough.tile.data(), rough.origin.data()};
    CHECK(smpc_robot_sim_set_terrain(twin.handle(), &t) == 0);
  }
  {
    const Sim::TerrainDevice d = sim.terrainDevicePointers();
    CHECK(d.heights != nullptr && d.tile != nullptr && d.origin != nullptr && d.nx == TNX && d.ny == TNY && d.tiles == 2 && d.cell == cell);
  }
  Sim level(robot, 3, B);
  level.setGround(gs);
  level.setTerrain(flat);
  {
    DeviceBuffer Xa(X), Xb(X), Xc(X), Xd(X), td(tau);
    for (int k = 0; k < steps; k++)
    {
      sim.stepGroundDevice(Xa.p, td.p, dt);
      twin.stepGroundDevice(Xb.p, td.p, dt);
      plain.stepGroundDevice(Xc.p, td.p, dt);
      level.stepGroundDevice(Xd.p, td.p, dt);
      sim.wait();
      twin.wait();
      plain.wait();
      level.wait();
      CHECK(Xa.get() == Xb.get() && sim.lastGroundForces() == twin.lastGroundForces() && sim.lastAccelerations() == twin.lastAccelerations());
      CHECK(sim.lastTerrainNormals() == twin.lastTerrainNormals() && sim.lastTerrainHeights() == twin.lastTerrainHeights());
      CHECK(Xc.get() == Xd.get() && plain.lastGroundForces() == level.lastGroundForces() && plain.lastContacts() == level.lastContacts());
      CHECK(level.lastTerrainHeights() == std::vector<double>((size_t)B * 4, gz));
    }
    CHECK(!(Xa.get() == Xc.get()));
    const std::vector<double> n = sim.lastTerrainNormals(), f = sim.lastGroundForces();
    double tilted = 0.0, fx = 0.0;
    for (size_t k = 0; k < n.size(); k += 3)
    {
      tilted = std::fmax(tilted, std::fabs(n[k]));
      fx = std::fmax(fx, std::fabs(f[k]));
    }
    std::printf("after %d steps on the rough tile: largest |n.x| under a foot %.4f, largest horizontal force %.3f N\n", steps, tilted, fx);
    CHECK(tilted > 0.01 && fx > 0.0);
  }
  // ---- refusals: the field and the first offending index; the previous terrain stays ----
  {
    const Sim::TerrainDevice before = sim.terrainDevicePointers();
    Sim::Terrain bad = rough;
    bad.heights[(size_t)(1 * TNY + 2) * TNX + 3] = NAN;
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("heights[1][2][3]") != std::string::npos);
    CHECK(refusal([&] { sim.groundTerrainDynamics(X, tau, dt, bad, model); }).find("heights[1][2][3]") != std::string::npos);
    bad = rough;
    bad.tile[2] = 2;
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("tile[2] = 2") != std::string::npos);
    bad = rough;
    bad.origin[3] = INFINITY;
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("origin[1][1]") != std::string::npos);
    bad = rough;
    bad.cell = 0.0;
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("cell") != std::string::npos);
    bad = rough;
    bad.heights[(size_t)(0 * TNY + 3) * TNX + 4] += 0.5;
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("slope[0][2][3]") != std::string::npos);
    bad = rough;
    bad.heights.pop_back();
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("heights [tiles][ny][nx]") != std::string::npos);
    bad = rough;
    bad.tile.pop_back();
    CHECK(refusal([&] { sim.setTerrain(bad); }).find("tile [rows]") != std::string::npos);
    const Sim::TerrainDevice after = sim.terrainDevicePointers();
    CHECK(after.heights == before.heights && after.tile == before.tile && after.origin == before.origin && after.nx == TNX);
  }
  // ---- cleared: the handle that never had any; setGround drops the terrain ----
  sim.clearTerrain();
  CHECK(sim.terrainDevicePointers().heights == nullptr);
  CHECK(refusal([&] { sim.lastTerrainNormals(); }).find("no terrain") != std::string::npos);
  twin.setGround(gs);
  CHECK(twin.terrainDevicePointers().heights == nullptr);
  Sim fresh(robot, 3, B);
  fresh.setGround(gs);
  {
    DeviceBuffer Xa(X), Xb(X), Xc(X), td(tau);
    for (int k = 0; k < 5; k++)
    {
      sim.stepGroundDevice(Xa.p, td.p, dt);
      twin.stepGroundDevice(Xb.p, td.p, dt);
      fresh.stepGroundDevice(Xc.p, td.p, dt);
    }
    sim.wait();
    twin.wait();
    fresh.wait();
    CHECK(Xa.get() == Xc.get() && Xb.get() == Xc.get());
  }
  std::printf("batched sim terrain mirror: OK\n");
  return 0;
}
