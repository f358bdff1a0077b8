"""Golden vectors of the ternary edge CEdgeP2CI3D at 50 digits:
    python tools/make_golden_bai_edges.py
evaluates tests/bai_ref.py (mpmath: Project_P2C, central differences at h = 1e-20 over the three documented increments)
on the cases of tests/bai_cases.edge_cases() and on a few CVertexIntrinsics::Operator_Plus updates, and stores inputs,
outputs rounded once to float64 and the branch rows in tests/golden/bai_edges.npz (data only)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bai_cases  # noqa: E402
import bai_ref  # noqa: E402

cams, intr, pts, obs = bai_cases.edge_cases()
out = [bai_ref.bai_edge(cams[int(o[0])], intr[int(o[2])], pts[int(o[1])], o[3:5]) for o in obs]
J2 = np.zeros((obs.shape[0], 12))
J2[:, :10] = np.array([o[2] for o in out])
rng = np.random.default_rng(7)
upd_v = np.array([[520.0, 480.0, 320.0, 240.0, 1e-3], [500.0, 505.0, 320.0, 240.0, 0.0], [1200.0, 1190.0, 640.0, 360.0, -2e-2],
                  [520.0, 480.0, 320.0, 240.0, 5.0]])
upd_d = np.concatenate([rng.normal(size=(3, 5)) * np.array([3.0, 3.0, 2.0, 2.0, 1e-3]), np.zeros((1, 5))])
upd_out = np.array([bai_ref.intrinsics_plus(v, d) for v, d in zip(upd_v, upd_d)])
dst = os.path.join(ROOT, "tests", "golden", "bai_edges.npz")
np.savez_compressed(dst, cams=cams, intr=intr, pts=pts, obs=obs, J0=np.array([o[0] for o in out]), J1=np.array([o[1] for o in out]),
                    J2=J2, r=np.array([o[3] for o in out]), aux=np.array([o[4] for o in out]),
                    branches=np.array([o[5] for o in out], dtype=np.int32), branch_names=np.array(bai_ref.BAI_BR),
                    upd_v=upd_v, upd_d=upd_d, upd_out=upd_out)
print(dst, obs.shape[0], "observations; branch rows:\n", np.array([o[5] for o in out]))
