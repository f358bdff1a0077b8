"""Golden vector of the reference application's Gauss-Newton loop on a 2D landmark graph:
    make -C oracle apps && python tools/make_golden_slam2d.py
writes the slam2d_small fixture as EDGE_SE2 / EDGE_SE2_RB lines, runs oracle/_ref/slam_plus_plus_ref -i <file> -nb -ns
(the reference's own parser, CEdgePose2D / CEdgePoseLandmark2D and CNonlinearSolver_Lambda, CPU only) and stores the
file's lines, the initial chi2 and the residual norms it prints, and its initial.txt / solution.txt states in
tests/golden/slam2d_gn.npz.

Two properties of the application shape the file: vertices must appear with ids in increasing order ("vertices must be
accessed in incremental manner"), so the vertices are renumbered by first appearance in the global edge order and no
VERTEX_SE2 lines are written -- poses come from composing the odometry, landmarks from
CRelative_to_Absolute_RangeBearing_Initializer, which stores (norm of a position, an angle) as the landmark. From that
start the five iterations do not converge; the golden pins the loop, not a solution."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_plus_plus_amd import synth  # noqa: E402

p = synth.make("slam2d_small")
edges = sorted([(q, 0, e) for e, q in enumerate(p.odo_seq)] + [(q, 1, e) for e, q in enumerate(p.obs_seq)])
ids = {}
lines = []
for _, kind, e in edges:
    row = p.obs[e] if kind else p.odo[e]
    a, b = (ids.setdefault(int(v), len(ids)) for v in row[:2])
    if kind:
        m = p.obs_info[e]
        lines.append("EDGE_SE2_RB %d %d %.17g %.17g %.17g %.17g %.17g" % (a, b, row[2], row[3], m[0, 0], m[0, 1], m[1, 1]))
    else:
        lines.append("EDGE_SE2 %d %d %.17g %.17g %.17g " % (a, b, row[2], row[3], row[4]) +
                     " ".join("%.17g" % x for x in p.odo_info[e][np.triu_indices(3)]))
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "slam2d.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "slam_plus_plus_ref"), "-i", path, "-nb", "-ns"], cwd=td,
                         env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, check=True).stdout
    flat = lambda name: np.concatenate([np.array(ln.split(), dtype=np.float64) for ln in open(os.path.join(td, name)) if ln.strip()])
    init, final = flat("initial.txt"), flat("solution.txt")
chi2 = float(re.search(r"initial denormalized chi2 error: ([0-9.eE+-]+)", out).group(1))
norms = np.array([float(x) for x in re.findall(r"residual norm: ([0-9.eE+-]+)", out)])
dst = os.path.join(ROOT, "tests", "golden", "slam2d_gn.npz")
np.savez_compressed(dst, lines=np.array(lines), initial_chi2=chi2, residual_norms=norms, init=init, final=final,
                    max_iter=5, threshold=0.01)
print(dst, len(lines), "edges, chi2", chi2, "norms", norms)
