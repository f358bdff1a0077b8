"""Golden vector of the reference application's Levenberg-Marquardt loop on a bundle adjustment with intrinsics vertices:
    make -C oracle apps && python tools/make_golden_bai.py
writes the bai_small fixture with formats.bai_lines (VERTEX_INTRINSICS / VERTEX_CAM / VERTEX_XYZ / EDGE_P2CI), runs
oracle/_ref/slam_plus_plus_ref -i <file> -nb -ns (the reference's own parser, CVertexCam / CVertexXYZ / CVertexIntrinsics,
the ternary CEdgeP2CI3D and CNonlinearSolver_Lambda_LM, CPU only; Main.cpp:192, 211 detects EDGE_P2CI in the file,
SolveBAIntrinsicsImpl.cpp solves it) and stores the file's lines, the initial and final chi2 and the per-iteration output
it prints, and its initial.txt / solution.txt states in tests/golden/bai_lm.npz (data only).

The application wants vertices to appear with ids in increasing order: the fixture numbers the intrinsics 0..1, the
cameras 2..7 and the points 8..47, and bai_lines writes the vertex lines in id order in front of the edges."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slam_plus_plus_amd import formats, synth  # noqa: E402

g = synth.make("bai_small").geometry
ids = np.concatenate([g["intr_id"], g["cam_id"], g["pt_id"]])
assert np.array_equal(ids, np.arange(ids.size))
lines = formats.bai_lines(g["cams"], g["intr"], g["points"], g["obs"], g["info"], g["cam_id"], g["pt_id"], g["intr_id"])
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "bai.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    run = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "slam_plus_plus_ref"), "-i", path, "-nb", "-ns"], cwd=td,
                         env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True)
    out = run.stdout
    if run.returncode != 0 or "chi2" not in out:
        sys.exit("the application refused the file:\n" + out + run.stderr)
    rows = lambda name: [np.array(ln.split(), dtype=np.float64) for ln in open(os.path.join(td, name)) if ln.strip()]
    init, final = rows("initial.txt"), rows("solution.txt")
chi2 = [float(x) for x in re.findall(r"denormalized chi2 error: ([0-9.eE+-]+)", out)]
iters = [ln for ln in out.splitlines() if re.search(r"residual norm|chi2|iteration|damping|alpha", ln)]
dim = np.array([r.size for r in init], dtype=np.int32)
dst = os.path.join(ROOT, "tests", "golden", "bai_lm.npz")
np.savez_compressed(dst, lines=np.array(lines), initial_chi2=chi2[0], final_chi2=chi2[-1], output=np.array(iters), dim=dim,
                    init=np.concatenate(init), final=np.concatenate(final), max_iter=5, threshold=0.01)
print(out)
print(dst, len(lines), "lines, chi2", chi2, "widths", np.bincount(dim))
