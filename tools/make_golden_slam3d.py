"""Golden vector of the reference application's Gauss-Newton loop on a 3D landmark graph:
    make -C oracle apps && python tools/make_golden_slam3d.py
writes the slam3d_small fixture as EDGE3:AXISANGLE / EDGE_SE3_XYZ lines, runs oracle/_ref/slam_plus_plus_ref -i <file> -nb -ns
(the reference's own parser, CEdgePose3D / CEdgePoseLandmark3D and CNonlinearSolver_Lambda, CPU only; Main.cpp:167-175
detects the 3D landmarks and takes the SE(3) solver) and stores the file's lines, the initial chi2 and the residual norms
it prints, and its initial.txt / solution.txt states in tests/golden/slam3d_gn.npz.

The application wants vertices to appear with ids in increasing order ("vertices must be accessed in incremental
manner"), so the vertices are renumbered by first appearance in the global edge order and no vertex lines are written:
poses come from composing the odometry, landmarks from CRelative_to_Absolute_XYZ_Initializer (t + R z)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_plus_plus_amd import formats, synth  # noqa: E402

p = synth.make("slam3d_small")
edges = sorted([(q, 0, e) for e, q in enumerate(p.odo_seq)] + [(q, 1, e) for e, q in enumerate(p.obs_seq)])
ids = {}
for _, kind, e in edges:
    for v in (p.obs[e] if kind else p.odo[e])[:2]:
        ids.setdefault(int(v), len(ids))
lines = formats.slam3d_lines(p.odo, p.odo_info, p.obs, p.obs_info, p.odo_seq, p.obs_seq, ids)
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "slam3d.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "slam_plus_plus_ref"), "-i", path, "-nb", "-ns"], cwd=td,
                         env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True)
    out = run.stdout
    if run.returncode != 0 or "residual norm" not in out:
        sys.exit("the application refused the file:\n" + out + run.stderr)
    rows = lambda name: [np.array(ln.split(), dtype=np.float64) for ln in open(os.path.join(td, name)) if ln.strip()]
    init, final = rows("initial.txt"), rows("solution.txt")
chi2 = float(re.search(r"initial denormalized chi2 error: ([0-9.eE+-]+)", out).group(1))
norms = np.array([float(x) for x in re.findall(r"residual norm: ([0-9.eE+-]+)", out)])
dim = np.array([r.size for r in init], dtype=np.int32)
dst = os.path.join(ROOT, "tests", "golden", "slam3d_gn.npz")
np.savez_compressed(dst, lines=np.array(lines), initial_chi2=chi2, residual_norms=norms, dim=dim, init=np.concatenate(init),
                    final=np.concatenate(final), max_iter=5, threshold=0.01)
print(out)
print(dst, len(lines), "edges, chi2", chi2, "norms", norms, "widths", np.bincount(dim))
