"""Compare two bench.py --dump-outputs directories array for array (bitwise): compare_dumps.py DIR_A DIR_B; exit
status 1 when any array differs."""
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
assert fa == fb, (fa, fb)
bad = 0
for f in fa:
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
    same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    print(f, x.shape, x.dtype, "identical" if same else "DIFFERENT")
    bad += not same
print("dumps:", "all identical" if not bad else f"{bad} differ", f"({len(fa)} arrays)")
sys.exit(1 if bad else 0)
