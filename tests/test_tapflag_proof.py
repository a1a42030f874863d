"""The NARROW brick kernels read "this +-delta tap sits in the centre tap's cell" from the fractions (csrc/dr_brick_common.h,
"tap-cell flags"): cell(p + delta) == cell(p) <=> fr+ >= fr, cell(p - delta) == cell(p) <=> fr- <= fr. tools/tapflag_proof.c
restates axis_coord on the host and checks both, and |cell(p +- delta) - cell(p)| <= 1, on every float position at the edges
2, 3, 13, 14, 25, 96, 256, 512, 990, 991 (recorded run: profiles/tapflags_proof.txt). This test compiles the same program and runs
its reduced set: all floats within 64 ulps of every position where q, q+ or q- is an integer and of the clamp points +-1,
+-(1 +- delta), and 10^7 random positions per edge."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [2, 3, 13, 14, 25, 96, 256, 512, 990, 991]


def test_fraction_flags_equal_cell_flags_at_the_narrow_edges(tmp_path):
    exe = str(tmp_path / "tapflag_proof")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", exe, os.path.join(ROOT, "tools", "tapflag_proof.c"), "-lm"])
    res = subprocess.run([exe, "reduced", "10000000"], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = re.findall(r"^reduced\s+edge\s+(\d+)\s.*positions\s+(\d+)\s+counter-examples (\d+)", res.stdout, re.M)
    assert [int(r[0]) for r in rows] == EDGES
    for edge, n, bad in rows:
        assert int(bad) == 0, (edge, bad)
        assert int(n) >= 10_000_000 + 3 * 129 * int(edge), (edge, n)   # the random positions + the windows around every integer crossing
    assert res.stdout.strip().endswith("OK")
    # ... and the check can fail: at an edge of 2001 voxels delta is a whole voxel, and a tap two cells on has fr+ >= fr
    res = subprocess.run([exe, "edge", "991", "2001"], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    found = dict((int(e), int(b)) for e, b in re.findall(r"^edge\s+edge\s+(\d+)\s.*counter-examples (\d+)", res.stdout, re.M))
    assert found[991] == 0 and found[2001] > 0, found
