"""Batch Gauss-Newton over the Lambda-solve hot path: the loop glue of the reference's
CNonlinearSolver_Lambda::Optimize (include/slam/NonlinearSolver_Lambda.h:539-666)
for 2D and 3D pose graphs. Product paths: `_ResidentPath` (the whole iteration in HBM: device
linearization, assembly, solve, ||dx||, vertex update) and `_DevicePath` (Jacobians on the host --
SURVEY 8d metric 2's baseline wording -- assembly and solve on the device).

Per iteration, exactly in the reference's order (:605-664):
    linearize at the current estimate  ->  Lambda = J^T Omega J (+ unary factor), eta = J^T Omega r
    dx = Lambda^-1 eta            (symbolic analysis once: the structure is fixed within Optimize)
    if ||dx|| <= f_min_dx_norm: stop WITHOUT applying dx
    x <- x (+) dx                 (CVertexPose2D::Operator_Plus, SE2_Types.h:70-74: add, clamp the angle)
    if the factorization failed: stop, estimate unchanged
Defaults are slam_app's: 5 iterations, threshold 0.01 (src/slam_app/Main.cpp:706-707).
"""
import collections
import math

import numpy as np

from . import api
from .formats import (se2_linearize, se3_linearize, se3_plus, ba_linearize, slam2d_linearize, slam2d_offsets,
                      slam3d_linearize, slam3d_offsets, slam3d_plus, stereo_linearize, bai_linearize, bai_intrinsics_plus,
                      bai_ids, BAI_INTR_WIDTH, rocv_linearize, sim3_ba_linearize, sim3_plus)


class CPoseGraph2D:
    """The 'system': vertex states (n, 3) x y theta, edges (m, 5) i j dx dy dtheta, information (m, 3, 3)."""

    def __init__(self, poses, edges, info):
        self.poses = np.array(poses, dtype=np.float64)
        self.edges = np.asarray(edges, dtype=np.float64)
        self.info = np.asarray(info, dtype=np.float64)

    dof = 3

    def linearize(self):
        return se2_linearize(self.poses, self.edges, self.info)

    def plus(self, dx):
        self.poses += dx.reshape(-1, 3)
        self.poses[:, 2] = np.fmod(self.poses[:, 2], 2 * math.pi)  # f_ClampAngle_2Pi, 2DSolverBase.h:44

    def chi2(self):
        prob = self.linearize()
        om = prob.Om.reshape(-1, 3, 3)
        return float(np.einsum("ei,eij,ej->", prob.r, om, prob.r))


class CPoseGraph3D:
    """3D pose graph: vertex states (n, 6) [t | axis-angle], edges (m, 8) i j + 6D measurement, information (m, 6, 6)
    (CVertexPose3D / CEdgePose3D, include/slam/SE3_Types.h)"""
    dof = 6

    def __init__(self, poses, edges, info):
        self.poses = np.array(poses, dtype=np.float64)
        self.edges = np.asarray(edges, dtype=np.float64)
        self.info = np.asarray(info, dtype=np.float64)

    def linearize(self):
        return se3_linearize(self.poses, self.edges, self.info)

    def plus(self, dx):
        self.poses = se3_plus(self.poses, dx.reshape(-1, 6))

    def chi2(self):
        prob = self.linearize()
        return float(np.einsum("ei,eij,ej->", prob.r, prob.Om.reshape(-1, 6, 6), prob.r))


class _SlamKind(collections.namedtuple("_SlamKind", "pose_w lm_w lin_odo lin_obs update listed")):
    """what tells 2D landmark SLAM from 3D: the widths of a pose and of a landmark (a measurement is as wide as what it
    measures: odometry pose_w columns, an observation lm_w, both after the two vertex ids), the api.Context methods that
    linearize the two edge groups and update the state, and the offsets the update lists beside the flat state (the
    system's attribute of that name)."""


_SLAM2D = _SlamKind(3, 2, "se2_linearize_at_device", "se2_rb_linearize_device", "slam2d_update_device", "angle_off")
_SLAM3D = _SlamKind(6, 3, "se3_linearize_at_device", "se3_xyz_linearize_device", "slam3d_update_device", "pose_off")


class _CSlam:
    """landmark SLAM 'system': poses and landmarks in one flat state laid out by `dim` (the layout of eta), odometry edges
    odo (m, 2 + pose_w) i j measurement + odo_info (m, pose_w, pose_w) and observations obs (k, 2 + lm_w) pose landmark
    measurement + obs_info (k, lm_w, lm_w). odo_seq / obs_seq: position of every edge in the graph's edge order (default:
    odometry, then observations). A subclass names its kind, its host linearization and its plus."""

    def __init__(self, dim, state, odo, odo_info, obs, obs_info, odo_seq=None, obs_seq=None, unary_vertex=0):
        self.dim = np.asarray(dim, dtype=np.int32)
        self.state = np.array(state, dtype=np.float64)
        self.odo, self.odo_info = np.asarray(odo, dtype=np.float64), np.asarray(odo_info, dtype=np.float64)
        self.obs, self.obs_info = np.asarray(obs, dtype=np.float64), np.asarray(obs_info, dtype=np.float64)
        m, k = self.odo.shape[0], self.obs.shape[0]
        self.odo_seq = np.arange(m, dtype=np.int64) if odo_seq is None else np.asarray(odo_seq, dtype=np.int64)
        self.obs_seq = m + np.arange(k, dtype=np.int64) if obs_seq is None else np.asarray(obs_seq, dtype=np.int64)
        self.unary_vertex = unary_vertex
        self.base = slam2d_offsets(self.dim)
        self.pose_off = self.base[:-1][self.dim == self.kind.pose_w]

    @classmethod
    def from_problem(cls, p):
        """from synth.slam2d_problem / slam3d_problem or formats.load_slam2d_graph / load_slam3d_graph"""
        return cls(p["dim"], p["state"], p["odo"], p["odo_info"], p["obs"], p["obs_info"], p.get("odo_seq"), p.get("obs_seq"),
                   p.get("unary_vertex", 0))

    def linearize(self):
        """the two edge groups (odometry, observations) as synth.Problems over the same vertices"""
        return self._linearize(self.dim, self.state, self.odo, self.odo_info, self.obs, self.obs_info, self.unary_vertex)

    def groups(self):
        p, l = self.kind.pose_w, self.kind.lm_w
        return [(self.odo[:, 0], self.odo[:, 1], p, p, p), (self.obs[:, 0], self.obs[:, 1], p, l, l)]

    def chi2(self):
        return float(sum(np.einsum("ei,eij,ej->", g.r, g.Om.reshape(-1, g.rd, g.rd), g.r) for g in self.linearize()))


class CSlam2D(_CSlam):
    """2D landmark SLAM: 3-wide poses and 2-wide landmarks (in 2D state and increment coincide), odometry dx dy dtheta
    (CEdgePose2D), observations range bearing (CEdgePoseLandmark2D)"""
    kind, _linearize = _SLAM2D, staticmethod(slam2d_linearize)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.angle_off = self.pose_off + 2

    def plus(self, dx):
        self.state += dx
        self.state[self.angle_off] = np.fmod(self.state[self.angle_off], 2 * math.pi)  # poses only (SE2_Types.h:70-74, :89)


class CSlam3D(_CSlam):
    """3D landmark SLAM: 6-wide poses [t | axis-angle] (the increment of a pose has 6 entries, too) and 3-wide landmarks,
    odometry t axis-angle (CEdgePose3D), observations x y z (CEdgePoseLandmark3D)"""
    kind, _linearize = _SLAM3D, staticmethod(slam3d_linearize)

    def plus(self, dx):
        self.state = slam3d_plus(self.dim, self.state, dx)  # poses composed, landmarks added (SE3_Types.h:44-47, :110-113)


class CRocv:
    """Range-only constant-velocity SLAM 'system' (src/slam_app/SolveROCVImpl.cpp), the interface of _CSlam: receivers
    [p | v] (6) and transmitters (3) in one flat state laid out by `dim`; constant-velocity edges cv (m, 3) i j dt + cv_info
    (m, 6, 6), ranges rng (k, 3) receiver transmitter range + rng_info (k,), priors on the transmitters pri (p,) + pri_info
    (p, 3, 3) -- unary edges --, and the position of every edge in the graph's edge order (default: the three groups one
    after the other). No built-in unary factor (CNullUnaryFactorFactory): the priors hold the graph."""
    unary_vertex = -1

    def __init__(self, dim, state, cv, cv_info, rng, rng_info, pri, pri_info, cv_seq=None, rng_seq=None, pri_seq=None):
        self.dim = np.asarray(dim, dtype=np.int32)
        self.state = np.array(state, dtype=np.float64)
        self.cv, self.cv_info = np.asarray(cv, dtype=np.float64).reshape(-1, 3), np.asarray(cv_info, dtype=np.float64)
        self.rng, self.rng_info = np.asarray(rng, dtype=np.float64).reshape(-1, 3), np.asarray(rng_info, dtype=np.float64)
        self.pri, self.pri_info = np.asarray(pri, dtype=np.int64).ravel(), np.asarray(pri_info, dtype=np.float64)
        m, k, p = self.cv.shape[0], self.rng.shape[0], self.pri.size
        self.cv_seq = np.arange(m, dtype=np.int64) if cv_seq is None else np.asarray(cv_seq, dtype=np.int64)
        self.rng_seq = m + np.arange(k, dtype=np.int64) if rng_seq is None else np.asarray(rng_seq, dtype=np.int64)
        self.pri_seq = m + k + np.arange(p, dtype=np.int64) if pri_seq is None else np.asarray(pri_seq, dtype=np.int64)
        self.base = slam2d_offsets(self.dim)

    @classmethod
    def from_problem(cls, p):
        """from synth.rocv_problem or formats.load_rocv_graph"""
        return cls(p["dim"], p["state"], p["cv"], p["cv_info"], p["rng"], p["rng_info"], p["pri"], p["pri_info"],
                   p.get("cv_seq"), p.get("rng_seq"), p.get("pri_seq"))

    def seqs(self):
        return [self.cv_seq, self.rng_seq, self.pri_seq]

    def linearize(self):
        """the three edge groups (constant velocity, ranges, priors) as synth.Problems over the same vertices"""
        return rocv_linearize(self.dim, self.state, self.cv, self.cv_info, self.rng, self.rng_info, self.pri, self.pri_info)

    def groups(self):
        return [(self.cv[:, 0], self.cv[:, 1], 6, 6, 6), (self.rng[:, 0], self.rng[:, 1], 6, 3, 1), (self.pri, None, 3, 0, 3)]

    def chi2(self):
        return float(sum(np.einsum("ei,eij,ej->", g.r, g.Om.reshape(-1, g.rd, g.rd), g.r) for g in self.linearize()))

    def plus(self, dx):
        self.state += dx   # both vertex types add plainly (ROCV_Types.h:60-63, CVertexLandmark3D)


class _Path:
    """what every product path has: its own api.Context, close(), and the symbolic analysis of self.st before the first
    factorization (FinalBlockStructure + symbolic: once per Optimize, the structure is fixed within it)"""

    def __init__(self, device=0):
        self.ctx = api.Context(device)
        self.st = None
        self.analyzed = False

    def _analyze_once(self):
        if not self.analyzed:
            self.ctx.analyze(self.st, api.MODE_AUTO)
            self.analyzed = True

    def close(self):
        self.ctx.close()


class _DeviceGroupsPath(_Path):
    """Jacobians on the host, multi-group device assembly + device solve (host_jacobians=True)"""

    def __init__(self, device=0, seq=None):
        super().__init__(device)
        self.seq = seq   # per group: the position of every edge in the graph's edge order (None: groups concatenated)

    def solve(self, groups, first):
        ctx = self.ctx
        if first:
            self.st = ctx.assemble_analyze_groups(groups[0].dim, [(g.v0, g.v1, g.d0, g.d1, g.rd) for g in groups],
                                                  self.seq, groups[0].unary_vertex)
            self.d_vals, self.d_eta = api.DeviceArray(ctx, self.st.nvals), api.DeviceArray(ctx, self.st.n)
            self.d_in = [[api.DeviceArray(ctx, a.size) for a in (g.J0, g.J1, g.Om, g.r)] for g in groups]
            self.analyzed = False
        for d4, g in zip(self.d_in, groups):
            for d, a in zip(d4, (g.J0, g.J1, g.Om, g.r)):
                d.upload(np.ascontiguousarray(a).ravel())
        ctx.assemble_groups_device(*[[d4[k].ptr for d4 in self.d_in] for k in range(4)], groups[0].damping, self.d_vals.ptr,
                                   self.d_eta.ptr)
        self._analyze_once()
        if ctx.factor_solve_device(self.d_vals.ptr, self.d_eta.ptr) != 0:
            return False, None
        return True, self.d_eta.download()


class _DevicePath(_DeviceGroupsPath):
    """_DeviceGroupsPath over the one edge group of a pose graph: spp_assemble_groups_device on a one-group plan runs the
    kernels of spp_assemble_device and returns their bits (tests/test_gpu_assemble_groups.py asserts it)"""

    def solve(self, prob, first):
        return super().solve([prob], first)


class _ResidentSlamPath(_Path):
    """the whole Gauss-Newton iteration of a CSlam2D / CSlam3D in HBM: the kind's two linearize kernels,
    spp_assemble_groups_device, analyze once, spp_factor_solve_device, the kind's update. Host traffic: the 8-byte norm per
    update call -- one in step() (the stopping test), one in apply() (the kernel's sibling entry points return it whenever
    they run), so 16 bytes and two stream synchronisations per applied iteration, as in _ResidentPath."""
    kind = None

    def begin(self, system):
        ctx, s, (pw, lw) = self.ctx, system, self.kind[:2]
        up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
        self.m, self.k, self.n = s.odo.shape[0], s.obs.shape[0], s.state.size
        self.st = ctx.assemble_analyze_groups(s.dim, s.groups(), [s.odo_seq, s.obs_seq], s.unary_vertex)
        off = lambda col: up(s.base[col.astype(np.int64)])
        self.d_off = [off(s.odo[:, 0]), off(s.odo[:, 1]), off(s.obs[:, 0]), off(s.obs[:, 1])]
        self.d_meas = [up(s.odo[:, 2:2 + pw]), up(s.obs[:, 2:2 + lw])]
        self.d_Om = [up(s.odo_info), up(s.obs_info)]
        listed = getattr(s, self.kind.listed)
        self.d_state, self.d_listed, self.n_listed = up(s.state), up(listed.astype(np.int64)), listed.size
        self.d_J0 = [api.DeviceArray(ctx, pw * pw * self.m), api.DeviceArray(ctx, lw * pw * self.k)]
        self.d_J1 = [api.DeviceArray(ctx, pw * pw * self.m), api.DeviceArray(ctx, lw * lw * self.k)]
        self.d_r = [api.DeviceArray(ctx, pw * self.m), api.DeviceArray(ctx, lw * self.k)]
        self.d_vals, self.d_eta = api.DeviceArray(ctx, self.st.nvals), api.DeviceArray(ctx, self.st.n)
        self._lin, self._upd = (getattr(ctx, self.kind.lin_odo), getattr(ctx, self.kind.lin_obs)), getattr(ctx, self.kind.update)
        self.analyzed = False

    def linearize(self):
        for g, (lin, n) in enumerate(zip(self._lin, (self.m, self.k))):
            lin(n, self.d_off[2 * g].ptr, self.d_off[2 * g + 1].ptr, self.d_state.ptr, self.d_meas[g].ptr,
                self.d_J0[g].ptr, self.d_J1[g].ptr, self.d_r[g].ptr)

    def chi2(self):
        """error at the current state: the sum over the groups (re-linearizes)"""
        self.linearize()
        return (self.ctx.edge_chi2_device(self.m, self.kind.pose_w, self.d_r[0].ptr, self.d_Om[0].ptr) +
                self.ctx.edge_chi2_device(self.k, self.kind.lm_w, self.d_r[1].ptr, self.d_Om[1].ptr))

    def _update(self, apply):
        return self._upd(self.n, self.d_state.ptr, self.d_eta.ptr, self.n_listed, self.d_listed.ptr, apply=apply)

    def step(self):
        ctx = self.ctx
        self.linearize()
        ptrs = lambda arrs: [a.ptr for a in arrs]
        ctx.assemble_groups_device(ptrs(self.d_J0), ptrs(self.d_J1), ptrs(self.d_Om), ptrs(self.d_r), 0.0,
                                   self.d_vals.ptr, self.d_eta.ptr)
        self._analyze_once()
        if ctx.factor_solve_device(self.d_vals.ptr, self.d_eta.ptr) != 0:
            return False, 0.0
        return True, self._update(False)

    def apply(self):
        self._update(True)

    def finish(self, system):
        system.state[:] = self.d_state.download()


class _ResidentSlam2DPath(_ResidentSlamPath):
    """(3,3,3) odometry and (3,2,2) range-bearing groups; the update lists the pose angles it clamps"""
    kind = _SLAM2D


class _ResidentSlam3DPath(_ResidentSlamPath):
    """(6,6,6) odometry and (6,3,3) landmark groups; the update lists the poses it composes"""
    kind = _SLAM3D


class _ResidentROCVPath(_Path):
    """the whole Gauss-Newton iteration of a CRocv in HBM: spp_rocv_cv_linearize_device and spp_rocv_range_linearize_device,
    the priors' constants (J = I, r = 0, uploaded once), spp_assemble_groups_device over the three groups, analyze once,
    spp_factor_solve_device, spp_slam2d_update_device without angles (the plain sum). Host traffic as in
    _ResidentSlamPath. mode: MODE_AUTO takes the Schur mode (widths {6, 3}), which eliminates the handful of transmitters
    and leaves a dense reduced system over ALL receivers; the sparse mode sees a chain with a few dense columns ordered
    last and is the default."""

    def __init__(self, device=0, mode=api.MODE_SPARSE):
        super().__init__(device)
        self.mode = mode

    def _analyze_once(self):
        if not self.analyzed:
            self.ctx.analyze(self.st, self.mode)
            self.analyzed = True

    def begin(self, system):
        ctx, s = self.ctx, system
        up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
        self.m, self.k, self.p, self.n = s.cv.shape[0], s.rng.shape[0], s.pri.size, s.state.size
        self.st = ctx.assemble_analyze_groups(s.dim, s.groups(), s.seqs(), s.unary_vertex)
        off = lambda col: up(s.base[col.astype(np.int64)])
        self.d_off = [off(s.cv[:, 0]), off(s.cv[:, 1]), off(s.rng[:, 0]), off(s.rng[:, 1])]
        self.d_meas = [up(s.cv[:, 2]), up(s.rng[:, 2])]
        self.d_state = up(s.state)
        m, k, p = self.m, self.k, self.p
        self.d_Om = [up(s.cv_info), up(s.rng_info), up(s.pri_info)]
        self.d_J0 = [api.DeviceArray(ctx, 36 * m), api.DeviceArray(ctx, 6 * k), up(np.tile(np.eye(3).ravel(), (p, 1)))]
        self.d_J1 = [api.DeviceArray(ctx, 36 * m), api.DeviceArray(ctx, 3 * k), None]
        self.d_r = [api.DeviceArray(ctx, 6 * m), api.DeviceArray(ctx, k), up(np.zeros(3 * p))]
        self.d_vals, self.d_eta = api.DeviceArray(ctx, self.st.nvals), api.DeviceArray(ctx, self.st.n)
        self.analyzed = False

    def linearize(self):
        ctx = self.ctx
        ctx.rocv_cv_linearize_device(self.m, self.d_off[0].ptr, self.d_off[1].ptr, self.d_state.ptr, self.d_meas[0].ptr,
                                     self.d_J0[0].ptr, self.d_J1[0].ptr, self.d_r[0].ptr)
        ctx.rocv_range_linearize_device(self.k, self.d_off[2].ptr, self.d_off[3].ptr, self.d_state.ptr, self.d_meas[1].ptr,
                                        self.d_J0[1].ptr, self.d_J1[1].ptr, self.d_r[1].ptr)

    def chi2(self):
        """error at the current state (re-linearizes); the priors' chi2 is 0 (ROCV_Types.h:316-319)"""
        self.linearize()
        return (self.ctx.edge_chi2_device(self.m, 6, self.d_r[0].ptr, self.d_Om[0].ptr) +
                self.ctx.edge_chi2_device(self.k, 1, self.d_r[1].ptr, self.d_Om[1].ptr))

    def assemble(self):
        ptrs = lambda arrs: [None if a is None else a.ptr for a in arrs]
        self.ctx.assemble_groups_device(ptrs(self.d_J0), ptrs(self.d_J1), ptrs(self.d_Om), ptrs(self.d_r), 0.0,
                                        self.d_vals.ptr, self.d_eta.ptr)

    def step(self):
        self.linearize()
        self.assemble()
        self._analyze_once()
        if self.ctx.factor_solve_device(self.d_vals.ptr, self.d_eta.ptr) != 0:
            return False, 0.0
        return True, self._update(False)

    def _update(self, apply):
        return self.ctx.slam2d_update_device(self.n, self.d_state.ptr, self.d_eta.ptr, 0, None, apply=apply)

    def apply(self):
        self._update(True)

    def finish(self, system):
        system.state[:] = self.d_state.download()


class _ResidentPath(_Path):
    """the whole Gauss-Newton iteration in HBM: linearization (spp_se2_linearize_device), assembly, solve,
    ||dx|| and the vertex update (spp_se2_update_device). Host traffic per iteration: 8 bytes (the norm)."""

    def begin(self, system):
        ctx = self.ctx
        prob = system.linearize()   # only for the (constant) structure + Omega
        self.nv, self.ne, self.dof = system.poses.shape[0], system.edges.shape[0], system.dof
        self.st = ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, self.dof, self.dof, self.dof, prob.unary_vertex)
        self._lin = ctx.se2_linearize_device if self.dof == 3 else ctx.se3_linearize_device
        self._upd = ctx.se2_update_device if self.dof == 3 else ctx.se3_update_device
        self.d_v0 = api.DeviceArray.from_host(ctx, prob.v0.astype(np.int32))
        self.d_v1 = api.DeviceArray.from_host(ctx, prob.v1.astype(np.int32))
        self.d_meas = api.DeviceArray.from_host(ctx, np.ascontiguousarray(system.edges[:, 2:2 + self.dof]).ravel())
        self.d_poses = api.DeviceArray.from_host(ctx, system.poses.ravel())
        self.d_Om = api.DeviceArray.from_host(ctx, np.ascontiguousarray(prob.Om).ravel())
        dd = self.dof * self.dof
        self.d_J0, self.d_J1 = api.DeviceArray(ctx, dd * self.ne), api.DeviceArray(ctx, dd * self.ne)
        self.d_r = api.DeviceArray(ctx, self.dof * self.ne)
        self.d_vals, self.d_eta = api.DeviceArray(ctx, self.st.nvals), api.DeviceArray(ctx, self.st.n)
        self.analyzed = False

    def step(self):
        """linearize + assemble + solve; returns (ok, ||dx||); dx stays on the device"""
        ctx = self.ctx
        self._lin(self.ne, self.d_v0.ptr, self.d_v1.ptr, self.d_poses.ptr, self.d_meas.ptr,
                  self.d_J0.ptr, self.d_J1.ptr, self.d_r.ptr)
        ctx.assemble_device(self.d_J0.ptr, self.d_J1.ptr, self.d_Om.ptr, self.d_r.ptr, 0.0, self.d_vals.ptr, self.d_eta.ptr)
        self._analyze_once()
        if ctx.factor_solve_device(self.d_vals.ptr, self.d_eta.ptr) != 0:
            return False, 0.0
        return True, self._upd(self.nv, self.d_poses.ptr, self.d_eta.ptr, apply=False)

    def apply(self):
        self._upd(self.nv, self.d_poses.ptr, self.d_eta.ptr, apply=True)

    def finish(self, system):
        system.poses[:] = self.d_poses.download().reshape(-1, self.dof)


class CNonlinearSolver_Lambda:
    """mirror of the reference class for CPoseGraph2D systems. `path` may be replaced by any object with
    solve(problem, first) -> (ok, dx) (the tests drive the loop glue with a CPU checker that way)."""

    def __init__(self, system, path=None, device=0, verbose=False, host_jacobians=False):
        self.system = system
        if path is None:  # the product paths need the GPU; host_jacobians keeps the linearization in numpy
            if isinstance(system, CRocv):
                path = _DeviceGroupsPath(device, system.seqs()) if host_jacobians else _ResidentROCVPath(device)
            elif isinstance(system, _CSlam):
                resident = _ResidentSlam2DPath if isinstance(system, CSlam2D) else _ResidentSlam3DPath
                path = _DeviceGroupsPath(device, [system.odo_seq, system.obs_seq]) if host_jacobians else resident(device)
            else:
                path = _DevicePath(device) if host_jacobians else _ResidentPath(device)
        self.path = path
        self.verbose = verbose
        self.n_iterations = 0
        self.last_dx_norm = None

    def Optimize(self, n_max_iteration_num=5, f_min_dx_norm=0.01):
        s = self.system
        self.n_iterations = 0
        if hasattr(self.path, "step"):  # device-resident iteration
            self.path.begin(s)
            for it in range(n_max_iteration_num):
                ok, norm = self.path.step()
                self.n_iterations = it + 1
                self.last_dx_norm = norm
                if self.verbose:
                    print("%s, residual norm: %.4f" % ("Cholesky succeeded" if ok else "Cholesky failed", norm))
                if norm <= f_min_dx_norm or not ok:
                    break
                self.path.apply()
            self.path.finish(s)
            return self.n_iterations
        for it in range(n_max_iteration_num):
            prob = s.linearize()
            ok, dx = self.path.solve(prob, it == 0)
            self.n_iterations = it + 1
            norm = float(np.linalg.norm(dx)) if ok else 0.0
            self.last_dx_norm = norm
            if self.verbose:
                print("%s, residual norm: %.4f" % ("Cholesky succeeded" if ok else "Cholesky failed", norm))
            if norm <= f_min_dx_norm:
                break
            if ok:
                s.plus(dx)
            else:
                break
        return self.n_iterations


# --------------------------------------------------------------------------------------------------
# Levenberg-Marquardt (what slam_app silently uses for every BA input, src/slam_app/Main.cpp:203-208)
# --------------------------------------------------------------------------------------------------
class CBundleAdjustment:
    """BA 'system': cams (nc, 6) [t | axis-angle] world -> camera, intr (nc, 5), points (np, 3), obs (no, 4)
    cam pt u v. Vertex ids: cameras 0..nc-1, points nc.. (the layout of the reference's BA example)."""

    def __init__(self, cams, intr, points, obs):
        self.cams = np.array(cams, dtype=np.float64)
        self.intr = np.asarray(intr, dtype=np.float64)
        self.points = np.array(points, dtype=np.float64)
        self.obs = np.asarray(obs, dtype=np.float64)

    def linearize(self):
        return ba_linearize(self.cams, self.intr, self.points, self.obs)

    def chi2(self):
        r = self.linearize().r
        return float((r ** 2).sum())

    def state(self):
        return self.cams.copy(), self.points.copy()

    def set_state(self, st):
        self.cams, self.points = st[0].copy(), st[1].copy()

    def plus(self, dx):
        nc = self.cams.shape[0]
        self.cams = se3_plus(self.cams, dx[:6 * nc].reshape(nc, 6))
        self.points = self.points + dx[6 * nc:].reshape(-1, 3)


class _ResidentBAPath(_Path):
    """LM iteration pieces in HBM: spp_ba_linearize_device, spp_assemble_device (damping alpha),
    spp_factor_solve_device, spp_ba_update_device, chi2 / alpha0 / gain-ratio reductions. A subclass overrides what its
    edge differs in: rd / n_ids, _analyze_structure, _dx_offsets, _begin_extra, linearize, _assemble, max_hessian_diag, and
    extends save / restore / apply / finish for a further vertex set."""
    rd = 2                                  # residual dimension: the edge group is (cam_w, 3, rd)
    cam_w = 6                               # width of a camera vertex (7: _ResidentSim3BAPath)
    n_ids = 2                               # obs starts with that many vertex ids (cam pt); the measurement follows

    def _analyze_structure(self, prob):
        return self.ctx.assemble_analyze(prob.dim, prob.v0, prob.v1, self.cam_w, 3, self.rd, prob.unary_vertex)

    def _dx_offsets(self, s):
        """scalar offsets of the cameras and of the points in the solution vector: cameras first"""
        w = self.cam_w
        return w * np.arange(self.nc, dtype=np.int64), w * self.nc + 3 * np.arange(self.np, dtype=np.int64)

    def _begin_extra(self, s, up):
        """device arrays of a further vertex set"""

    def begin(self, system):
        ctx, s = self.ctx, system
        prob = s.linearize()   # structure only
        self.no, self.nc, self.np = s.obs.shape[0], s.cams.shape[0], s.points.shape[0]
        rd = self.rd
        self.st = self._analyze_structure(prob)
        up = lambda a: api.DeviceArray.from_host(ctx, np.ascontiguousarray(a).ravel())
        self.d_cam_of, self.d_pt_of = up(s.obs[:, 0].astype(np.int32)), up(s.obs[:, 1].astype(np.int32))
        self.d_cams, self.d_intr, self.d_pts = up(s.cams), up(s.intr), up(s.points)
        self.d_meas, self.d_Om = up(s.obs[:, self.n_ids:self.n_ids + rd]), up(prob.Om)
        cam_off, pt_off = self._dx_offsets(s)
        self.d_cam_off, self.d_pt_off = up(cam_off), up(pt_off)
        self.d_J0, self.d_J1 = api.DeviceArray(ctx, self.cam_w * rd * self.no), api.DeviceArray(ctx, 3 * rd * self.no)
        self.d_r = api.DeviceArray(ctx, rd * self.no)
        self.d_vals, self.d_eta, self.d_dx = (api.DeviceArray(ctx, self.st.nvals), api.DeviceArray(ctx, self.st.n),
                                              api.DeviceArray(ctx, self.st.n))
        self.s_cams, self.s_pts = api.DeviceArray(ctx, self.cam_w * self.nc), api.DeviceArray(ctx, 3 * self.np)
        self._begin_extra(s, up)
        self.analyzed = False

    def linearize(self):
        self.ctx.ba_linearize_device(self.no, self.d_cam_of.ptr, self.d_pt_of.ptr, self.d_cams.ptr, self.d_intr.ptr,
                                     self.d_pts.ptr, self.d_meas.ptr, self.d_J0.ptr, self.d_J1.ptr, self.d_r.ptr)

    def chi2(self):
        """error at the CURRENT state (re-evaluates the residuals; J of the last linearization is overwritten too,
        which the loop accounts for by re-linearizing after a rejected step is rolled back)"""
        self.linearize()
        return self.ctx.edge_chi2_device(self.no, self.rd, self.d_r.ptr, self.d_Om.ptr)

    def max_hessian_diag(self):
        return self.ctx.edge_hessian_maxdiag_device(self.no, self.rd, self.cam_w, 3, self.d_J0.ptr, self.d_J1.ptr, self.d_Om.ptr)

    def _assemble(self, alpha):
        self.ctx.assemble_device(self.d_J0.ptr, self.d_J1.ptr, self.d_Om.ptr, self.d_r.ptr, alpha, self.d_vals.ptr,
                                 self.d_eta.ptr)

    def _update(self, apply):
        """cameras and points (+) dx; returns ||dx|| over the whole solution vector"""
        return self.ctx.ba_update_device(self.nc, self.d_cams.ptr, self.d_cam_off.ptr, self.np, self.d_pts.ptr,
                                         self.d_pt_off.ptr, self.d_dx.ptr, self.st.n, apply=apply)

    def solve(self, alpha):
        self._assemble(alpha)
        self._analyze_once()
        self.d_dx.copy_from(self.d_eta)
        if self.ctx.factor_solve_device(self.d_vals.ptr, self.d_dx.ptr) != 0:
            return False, 0.0
        return True, self._update(False)

    def gain_denominator(self, alpha):
        return self.ctx.lm_gain_denominator_device(self.st.n, self.d_dx.ptr, self.d_eta.ptr, alpha)

    def save(self):
        self.s_cams.copy_from(self.d_cams)
        self.s_pts.copy_from(self.d_pts)

    def restore(self):
        self.d_cams.copy_from(self.s_cams)
        self.d_pts.copy_from(self.s_pts)

    def apply(self):
        self._update(True)

    def finish(self, system):
        system.cams = self.d_cams.download().reshape(-1, self.cam_w)
        system.points = self.d_pts.download().reshape(-1, 3)


class CStereoBundleAdjustment:
    """Stereo BA 'system' (CVertexSCam + CVertexXYZ joined by CEdgeP2SC3D, src/slam_app/SolveBAStereoImpl.cpp), the
    interface of CBundleAdjustment: cams (nc, 6) [t | axis-angle] world -> left camera, intr (nc, 6) fx fy cx cy d b,
    points (np, 3), obs (no, 5) cam pt u v u_right; info (no, 3, 3) or None (identity). Vertex ids: cameras 0..nc-1, points
    nc.. unless cam_id / pt_id say otherwise (a graph file may interleave them)."""

    def __init__(self, cams, intr, points, obs, info=None, cam_id=None, pt_id=None):
        self.cams = np.array(cams, dtype=np.float64)
        self.intr = np.asarray(intr, dtype=np.float64)
        self.points = np.array(points, dtype=np.float64)
        self.obs = np.asarray(obs, dtype=np.float64)
        self.info = None if info is None else np.asarray(info, dtype=np.float64)
        nc, npts = self.cams.shape[0], self.points.shape[0]
        self.cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id, dtype=np.int64)
        self.pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id, dtype=np.int64)
        dim = np.empty(nc + npts, dtype=np.int64)
        dim[self.cam_id], dim[self.pt_id] = 6, 3
        base = slam3d_offsets(dim)
        self.cam_off, self.pt_off = base[self.cam_id], base[self.pt_id]   # scalar offsets in the solution vector

    @classmethod
    def from_problem(cls, p):
        """from synth.stereo_problem (its geometry) or formats.load_stereo_graph"""
        g = p["geometry"] if "geometry" in p else p
        return cls(g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"])

    def linearize(self):
        return stereo_linearize(self.cams, self.intr, self.points, self.obs, self.cam_id, self.pt_id, self.info)

    def chi2(self):
        p = self.linearize()
        return float(np.einsum("ei,eij,ej->", p.r, p.Om.reshape(-1, 3, 3), p.r))

    def state(self):
        return self.cams.copy(), self.points.copy()

    def set_state(self, st):
        self.cams, self.points = st[0].copy(), st[1].copy()

    def plus(self, dx):
        """CVertexSCam::Operator_Plus is Relative_to_Absolute (BA_Types.h:264-267), CVertexXYZ's the plain sum"""
        self.cams = se3_plus(self.cams, dx[self.cam_off[:, None] + np.arange(6)])
        self.points = self.points + dx[self.pt_off[:, None] + np.arange(3)]


class _ResidentStereoBAPath(_ResidentBAPath):
    """the LM iteration pieces of a CStereoBundleAdjustment in HBM: _ResidentBAPath with the (6, 3, 3) group --
    assemble_analyze(..., 6, 3, 3, ...), spp_ba_stereo_linearize_device, edge_chi2_device(no, 3, ...),
    edge_hessian_maxdiag_device(no, 3, 6, 3, ...) -- and spp_ba_update_device as it is, the vertices at the system's
    offsets."""
    rd = 3

    def _dx_offsets(self, s):
        return s.cam_off.astype(np.int64), s.pt_off.astype(np.int64)

    def linearize(self):
        self.ctx.ba_stereo_linearize_device(self.no, self.d_cam_of.ptr, self.d_pt_of.ptr, self.d_cams.ptr, self.d_intr.ptr,
                                            self.d_pts.ptr, self.d_meas.ptr, self.d_J0.ptr, self.d_J1.ptr, self.d_r.ptr)


class CBundleAdjustmentSim3:
    """Sim(3) BA 'system' (CVertexCamSim3 + CVertexXYZ joined by CEdgeP2C_XYZ_Sim3_G, the observation of the reference's
    ba_parameter_acra and incremental_ba_3dv), the interface of CStereoBundleAdjustment: cams (nc, 7) [t | w | s] in sim(3),
    intr (nc, 5) fx fy cx cy d, points (np, 3), obs (no, 4) cam pt u v; info (no, 2, 2) or None (identity). Sim(3) BA has
    seven gauge freedoms and a scale per camera that the projection does not see (the scale column of J0 is zero): the
    damping of Levenberg-Marquardt is what makes Lambda definite, CNonlinearSolver_Lambda_LM is the loop to use."""

    def __init__(self, cams, intr, points, obs, info=None, cam_id=None, pt_id=None):
        self.cams = np.array(cams, dtype=np.float64)
        self.intr = np.asarray(intr, dtype=np.float64)
        self.points = np.array(points, dtype=np.float64)
        self.obs = np.asarray(obs, dtype=np.float64)
        self.info = None if info is None else np.asarray(info, dtype=np.float64)
        nc, npts = self.cams.shape[0], self.points.shape[0]
        self.cam_id = np.arange(nc) if cam_id is None else np.asarray(cam_id, dtype=np.int64)
        self.pt_id = nc + np.arange(npts) if pt_id is None else np.asarray(pt_id, dtype=np.int64)
        dim = np.empty(nc + npts, dtype=np.int64)
        dim[self.cam_id], dim[self.pt_id] = 7, 3
        base = slam3d_offsets(dim)
        self.cam_off, self.pt_off = base[self.cam_id], base[self.pt_id]   # scalar offsets in the solution vector

    @classmethod
    def from_problem(cls, p):
        """from synth.sim3_problem (its geometry) or formats.load_sim3_graph"""
        g = p["geometry"] if "geometry" in p else p
        return cls(g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"])

    def linearize(self):
        return sim3_ba_linearize(self.cams, self.intr, self.points, self.obs, self.cam_id, self.pt_id, self.info)

    def chi2(self):
        p = self.linearize()
        return float(np.einsum("ei,eij,ej->", p.r, p.Om.reshape(-1, 2, 2), p.r))

    def state(self):
        return self.cams.copy(), self.points.copy()

    def set_state(self, st):
        self.cams, self.points = st[0].copy(), st[1].copy()

    def plus(self, dx):
        """CVertexCamSim3::Operator_Plus: Log(Exp(cam) Exp(d)); CVertexXYZ's the plain sum"""
        self.cams = sim3_plus(self.cams, dx[self.cam_off[:, None] + np.arange(7)])
        self.points = self.points + dx[self.pt_off[:, None] + np.arange(3)]


class _ResidentSim3BAPath(_ResidentBAPath):
    """the LM iteration pieces of a CBundleAdjustmentSim3 in HBM: _ResidentBAPath with the (7, 3, 2) group --
    assemble_analyze(..., 7, 3, 2, ...), spp_sim3_ba_linearize_device, edge_hessian_maxdiag_device(no, 2, 7, 3, ...),
    spp_sim3_update_device --, the vertices at the system's offsets. host_jacobians=True: J0, J1 and r come from the float64
    mirror at the state downloaded from the device (formats.sim3_ba_linearize), everything else stays on the device."""
    cam_w = 7

    def __init__(self, device=0, host_jacobians=False):
        super().__init__(device)
        self.host_jacobians = host_jacobians

    def begin(self, system):
        super().begin(system)
        self.system = system

    def _dx_offsets(self, s):
        return s.cam_off.astype(np.int64), s.pt_off.astype(np.int64)

    def linearize(self):
        if self.host_jacobians:
            s = self.system
            p = sim3_ba_linearize(self.d_cams.download().reshape(-1, 7), s.intr, self.d_pts.download().reshape(-1, 3), s.obs,
                                  s.cam_id, s.pt_id, s.info)
            for d, a in ((self.d_J0, p.J0), (self.d_J1, p.J1), (self.d_r, p.r)):
                d.upload(np.ascontiguousarray(a).ravel())
            return
        self.ctx.sim3_ba_linearize_device(self.no, self.d_cam_of.ptr, self.d_pt_of.ptr, self.d_cams.ptr, self.d_intr.ptr,
                                          self.d_pts.ptr, self.d_meas.ptr, self.d_J0.ptr, self.d_J1.ptr, self.d_r.ptr)

    def _update(self, apply):
        return self.ctx.sim3_update_device(self.nc, self.d_cams.ptr, self.d_cam_off.ptr, self.np, self.d_pts.ptr,
                                           self.d_pt_off.ptr, self.d_dx.ptr, self.st.n, apply=apply)


class CBundleAdjustmentIntrinsics:
    """Self-calibrating BA 'system' (CVertexCam + CVertexXYZ + CVertexIntrinsics joined by the ternary CEdgeP2CI3D,
    src/slam_app/SolveBAIntrinsicsImpl.cpp), the interface of CBundleAdjustment: cams (nc, 6) [t | axis-angle] world ->
    camera, intr (ni, 5) fx fy cx cy kappa, points (np, 3), obs (no, 5) cam pt intr u v; info (no, 2, 2) or None (identity).
    Vertex ids: formats.bai_ids unless cam_id / pt_id / intr_id say otherwise. The increment is PADDED: an intrinsics vertex
    takes 6 entries of dx, the last of them inert (zero)."""

    def __init__(self, cams, intr, points, obs, info=None, cam_id=None, pt_id=None, intr_id=None):
        self.cams = np.array(cams, dtype=np.float64)
        self.intr = np.array(intr, dtype=np.float64)
        self.points = np.array(points, dtype=np.float64)
        self.obs = np.asarray(obs, dtype=np.float64)
        self.info = None if info is None else np.asarray(info, dtype=np.float64)
        nc, npts, ni = self.cams.shape[0], self.points.shape[0], self.intr.shape[0]
        self.cam_id, self.pt_id, self.intr_id = bai_ids(nc, npts, ni, cam_id, pt_id, intr_id)
        dim = np.empty(nc + npts + ni, dtype=np.int64)
        dim[self.cam_id], dim[self.pt_id], dim[self.intr_id] = 6, 3, BAI_INTR_WIDTH
        base = slam3d_offsets(dim)
        self.cam_off, self.pt_off, self.intr_off = base[self.cam_id], base[self.pt_id], base[self.intr_id]

    @classmethod
    def from_problem(cls, p):
        """from synth.bai_problem (its geometry) or formats.load_bai_graph"""
        g = p["geometry"] if "geometry" in p else p
        return cls(g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"], g["intr_id"])

    def linearize(self):
        return bai_linearize(self.cams, self.intr, self.points, self.obs, self.cam_id, self.pt_id, self.intr_id, self.info)

    def chi2(self):
        p = self.linearize()
        return float(np.einsum("ei,eij,ej->", p.r, p.Om.reshape(-1, 2, 2), p.r))

    def state(self):
        return self.cams.copy(), self.points.copy(), self.intr.copy()

    def set_state(self, st):
        self.cams, self.points, self.intr = st[0].copy(), st[1].copy(), st[2].copy()

    def plus(self, dx):
        """cameras: Relative_to_Absolute; points: the plain sum; intrinsics: CVertexIntrinsics::Operator_Plus as written
        (formats.bai_intrinsics_plus) on the 5 live entries"""
        self.cams = se3_plus(self.cams, dx[self.cam_off[:, None] + np.arange(6)])
        self.points = self.points + dx[self.pt_off[:, None] + np.arange(3)]
        self.intr = bai_intrinsics_plus(self.intr, dx[self.intr_off[:, None] + np.arange(5)])


class _ResidentBAIPath(_ResidentBAPath):
    """the LM iteration pieces of a CBundleAdjustmentIntrinsics in HBM: states, J0 / J1 / J2, Lambda and the padded dx stay
    on the device -- spp_ba_intrinsics_linearize_device, spp_assemble_ternary_device (damping alpha), spp_factor_solve_device
    (AUTO: the dense Schur mode, poses = cameras + intrinsics), spp_ba_update_device for cameras and points (its norm runs
    over the padded dx, whose inert entries are zero) and spp_ba_intrinsics_update_device; chi2 and the gain denominator as
    in _ResidentBAPath, the initial damping from the larger of the (J0, J1) and (J2, J1) vertex Hessian diagonals. A rejected
    step restores cameras, points and intrinsics."""
    rd, n_ids = 2, 3                        # obs: cam pt intr u v

    def _analyze_structure(self, prob):
        return self.ctx.assemble_analyze_ternary(prob.dim, prob.v0, prob.v1, prob.v2, prob.unary_vertex)

    _dx_offsets = _ResidentStereoBAPath._dx_offsets   # the vertices at the system's offsets

    def _begin_extra(self, s, up):
        self.ni = s.intr.shape[0]
        self.d_intr_of, self.d_intr_off = up(s.obs[:, 2].astype(np.int32)), up(s.intr_off.astype(np.int64))
        self.d_J2, self.s_intr = api.DeviceArray(self.ctx, 12 * self.no), api.DeviceArray(self.ctx, 5 * self.ni)

    def linearize(self):
        self.ctx.ba_intrinsics_linearize_device(self.no, self.d_cam_of.ptr, self.d_pt_of.ptr, self.d_intr_of.ptr, self.d_cams.ptr,
                                                self.d_intr.ptr, self.d_pts.ptr, self.d_meas.ptr, self.d_J0.ptr, self.d_J1.ptr,
                                                self.d_J2.ptr, self.d_r.ptr)

    def max_hessian_diag(self):
        f = lambda d_J: self.ctx.edge_hessian_maxdiag_device(self.no, 2, 6, 3, d_J.ptr, self.d_J1.ptr, self.d_Om.ptr)
        return max(f(self.d_J0), f(self.d_J2))

    def _assemble(self, alpha):
        self.ctx.assemble_ternary_device(self.d_J0.ptr, self.d_J1.ptr, self.d_J2.ptr, self.d_Om.ptr, self.d_r.ptr, alpha,
                                         self.d_vals.ptr, self.d_eta.ptr)

    def save(self):
        super().save()
        self.s_intr.copy_from(self.d_intr)

    def restore(self):
        super().restore()
        self.d_intr.copy_from(self.s_intr)

    def apply(self):
        super().apply()
        self.ctx.ba_intrinsics_update_device(self.ni, self.d_intr.ptr, self.d_intr_off.ptr, self.d_dx.ptr, apply=True)

    def finish(self, system):
        super().finish(system)
        system.intr = self.d_intr.download().reshape(-1, 5)


class CNonlinearSolver_Lambda_LM:
    """Mirror of CNonlinearSolver_Lambda_LM::Optimize (include/slam/NonlinearSolver_Lambda_LM.h:796-1135) with
    the Levenberg trust-region policy of :151-222:
        alpha0 = 1e-3 * largest diagonal entry of any vertex Hessian;  last = chi2(x)
        loop: Lambda = J^T Omega J + alpha I (re-linearized only after an accepted step), dx = Lambda^-1 eta,
              stop if ||dx|| <= threshold; save x; x <- x (+) dx; err = chi2(x);
              rho = (last - err) / (dx . (alpha dx + eta));
              rho > 0: alpha *= max(1/3, 1 - (2 rho - 1)^3), nu = 2, last = err
              else   : alpha *= nu, nu *= 2, restore x, and the iteration budget grows by one (at most 10 times)
    `path`: _ResidentBAPath (default, GPU), _ResidentStereoBAPath for a CStereoBundleAdjustment, _ResidentBAIPath for a
    CBundleAdjustmentIntrinsics, _ResidentSim3BAPath for a CBundleAdjustmentSim3, or any object with the
    same methods (tests inject a host path)."""

    def __init__(self, system, path=None, device=0, verbose=False):
        self.system = system
        self.path = path if path is not None else _ResidentBAPath(device)
        self.verbose = verbose
        self.n_iterations = 0
        self.alpha = None
        self.chi2_history = []

    def Optimize(self, n_max_iteration_num=5, f_min_dx_norm=0.01):
        p = self.path
        p.begin(self.system)
        p.linearize()
        alpha = 1e-3 * p.max_hessian_diag()
        nu = 2.0
        last = p.chi2()
        self.chi2_history = [last]
        fail = 10
        dirty = False       # J / r on the device are those of the current state (chi2 re-linearized it)
        it = 0
        while it < n_max_iteration_num:
            if it and dirty:
                p.linearize()
            dirty = False
            ok, norm = p.solve(alpha)
            self.n_iterations = it + 1
            if not ok:
                break
            if self.verbose:
                print("iter %d: alpha %.6g ||dx|| %.6g" % (it, alpha, norm))
            if norm <= f_min_dx_norm:
                break
            p.save()
            denom = p.gain_denominator(alpha)
            p.apply()
            err = p.chi2()          # leaves J / r of the NEW state on the device
            rho = (last - err) / denom
            if rho > 0:
                alpha *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu = 2.0
                last = err
                self.chi2_history.append(err)
            else:
                alpha *= nu
                nu *= 2.0
                p.restore()
                dirty = True    # the device holds the linearization of the rejected state: redo it at the restored one
                if fail > 0:
                    fail -= 1
                    n_max_iteration_num += 1
            it += 1
        self.alpha = alpha
        p.finish(self.system)
        return self.n_iterations
