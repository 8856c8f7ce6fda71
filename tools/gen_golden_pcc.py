"""Writes tests/golden/pitch_pcc.npz: what the reference's prosody-transfer metric returns on a few dozen short curves.

Run where the reference tree and scipy are present:
    python tools/gen_golden_pcc.py <reference root>

`scripts/evaluation/compare_pitch_curves.py` of the reference is imported and `pcc_on_2_pitch_curve(ref, dut, remove_unvoiced)`
called on every pair; the resampled curve it forms on the way is recorded from the same module's `resample` (scipy's) applied to
its own `_remove_unvoiced`.  The fixture holds data only:
  remove (n,) bool, pcc (n,) float64, kept (n, 2) int64, and per pair i: ref<i>, dut<i> float32 inputs, resampled<i> float64.
The curves come from tests/curve_oracle.py (`voiced_pair`, `with_unvoiced`): log-Hz like, 5 +- 0.3, lengths 2 .. 150, with the
flag on (unvoiced runs of zeros and negative values in both curves) and off.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import curve_oracle as O  # noqa: E402

PAIRS = [(2, 2), (2, 5), (5, 2), (3, 3), (7, 4), (4, 7), (8, 8), (9, 8), (8, 9), (10, 12), (12, 10), (16, 15), (15, 16), (17, 31),
         (31, 17), (32, 32), (33, 47), (48, 33), (50, 50), (51, 64), (64, 51), (77, 100), (100, 77), (90, 91), (91, 90), (101, 101),
         (120, 60), (60, 120), (128, 150), (150, 128), (149, 97), (97, 149)]


def main(reference_root):
    path = os.path.join(reference_root, 'scripts', 'evaluation', 'compare_pitch_curves.py')
    spec = importlib.util.spec_from_file_location('compare_pitch_curves', path)
    cpc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cpc)
    out = {'remove': [], 'pcc': [], 'kept': []}
    for i, (nr, nd) in enumerate(PAIRS):
        remove = i % 2 == 0
        ref, dut = O.voiced_pair(nr, nd, 1000 + i)
        if remove:
            ref, dut = O.with_unvoiced(ref, 2000 + i), O.with_unvoiced(dut, 3000 + i)
        r64, d64 = ref.astype(np.float64), dut.astype(np.float64)
        pcc = float(cpc.pcc_on_2_pitch_curve(r64, d64, remove_unvoiced=remove))
        kr, kd = (cpc._remove_unvoiced(r64), cpc._remove_unvoiced(d64)) if remove else (r64, d64)
        assert len(kr) == nr and len(kd) == nd and np.isfinite(pcc)
        out['remove'].append(remove)
        out['pcc'].append(pcc)
        out['kept'].append((len(kr), len(kd)))
        out[f'ref{i}'], out[f'dut{i}'] = ref, dut
        out[f'resampled{i}'] = np.asarray(cpc.resample(kd, len(kr)), dtype=np.float64)
    out['remove'], out['pcc'], out['kept'] = np.array(out['remove']), np.array(out['pcc']), np.array(out['kept'], dtype=np.int64)
    dst = os.path.join(ROOT, 'tests', 'golden', 'pitch_pcc.npz')
    np.savez_compressed(dst, **out)
    print(f'{dst}: {len(PAIRS)} pairs, {os.path.getsize(dst)} bytes, pcc {out["pcc"].min():.3f} .. {out["pcc"].max():.3f}')


if __name__ == '__main__':
    main(sys.argv[1])
