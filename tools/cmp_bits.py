"""The two-process harness of the bit comparisons (cmp_beamformer_bits.py, cmp_em_bits.py).

A tool defines ``cases()`` -> {name: array} and ends with ``main(__file__, __doc__, cases)``.
``python TOOL OTHER_LIBRARY`` then runs the cases once under the package's own library and once
under OTHER_LIBRARY (GSS_HIP_LIBRARY), each in a process of its own (``python TOOL --run FILE``),
compares the arrays byte for byte and prints one line per array and the summary
"N arrays, M different".  Exit status 1 when an array differs."""
import os
import subprocess
import sys
import tempfile

import numpy as np


def main(tool, doc, cases):
    if len(sys.argv) == 3 and sys.argv[1] == '--run':
        np.savez(sys.argv[2], **cases())
        return
    if len(sys.argv) != 2:
        sys.exit(doc)
    tool = os.path.abspath(tool)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, 'a.npz'), os.path.join(tmp, 'b.npz')
        subprocess.run([sys.executable, tool, '--run', a], check=True)
        subprocess.run([sys.executable, tool, '--run', b], check=True,
                       env=dict(os.environ, GSS_HIP_LIBRARY=os.path.abspath(sys.argv[1])))
        A, B = np.load(a), np.load(b)
        different = 0
        for k in A.files:
            same = A[k].tobytes() == B[k].tobytes()
            different += not same
            print(k, 'bit-identical' if same else 'DIFFERENT max %.3e' % np.nanmax(np.abs(A[k] - B[k])),
                  'nan' if np.isnan(A[k]).any() else '')
        print(f'{len(A.files)} arrays, {different} different')
        sys.exit(1 if different else 0)
