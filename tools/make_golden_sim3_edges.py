"""Golden vectors of the Sim(3) projection edge CEdgeP2C_XYZ_Sim3_G and of CVertexCamSim3::Operator_Plus at 50 digits:
    python tools/make_golden_sim3_edges.py
evaluates tests/sim3_ref.py (mpmath: Exp from the closed forms of a, b, c, Log as its inverse, Project_P2C_XYZ, central
differences at h = 1e-20 over the post-multiplicative increment) on the cases of tests/sim3_cases.py, and stores inputs,
outputs rounded once to float64 and the branch rows in tests/golden/sim3_edges.npz (data only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_cases  # noqa: E402
import sim3_ref  # noqa: E402

cams, intr, pts, obs = sim3_cases.edge_cases()
out = [sim3_ref.sim3_edge(cams[int(o[0])], intr[int(o[0])], pts[int(o[1])], o[2:4]) for o in obs]
upd_v, upd_d = sim3_cases.update_cases()
upd = [sim3_ref.sim3_plus(v, d) for v, d in zip(upd_v, upd_d)]
dst = os.path.join(ROOT, "tests", "golden", "sim3_edges.npz")
np.savez_compressed(dst, cams=cams, intr=intr, pts=pts, obs=obs, J0=np.array([o[0] for o in out]), J1=np.array([o[1] for o in out]),
                    r=np.array([o[2] for o in out]), aux=np.array([o[3] for o in out]),
                    branches=np.array([o[4] for o in out], dtype=np.int32),
                    branch_names=np.array(["s cell", "w cell", "kappa = 0", "on the axis", "behind"]),
                    upd_v=upd_v, upd_d=upd_d, upd_out=np.array([u[0] for u in upd]), upd_R=np.array([u[1] for u in upd]),
                    upd_aux=np.array([u[2] for u in upd]))
print(dst, obs.shape[0], "observations,", upd_v.shape[0], "updates, %d bytes" % os.path.getsize(dst))
