#!/usr/bin/env python
"""Write tests/golden/ref_checkpoint.xz: a checkpoint written by the REFERENCE's own `save_checkpoint` (train.py:56-78) for its
DaftExprt at the default architecture (11 speakers, 193 tensors, 14.7 M parameters) after two `torch.optim.Adam` steps with the
reference trainer's settings (train.py:299-301), xz-compressed.  Imports the reference like tools/gen_goldens.py (same shims).

Weights and gradients are periodic per tensor (period 251 / 7 elements, offset by the tensor's index), so the 177 MB file
compresses to ~0.3 MB while every tensor still differs from every other and a transposed or reordered copy does not match.
tests/test_reference_interop.py loads it with this package's `load_checkpoint` and checks what this package writes against it.

Run:  python tools/gen_golden_checkpoint.py
"""
import lzma
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_checkpoint.xz')


def main():
    import gen_goldens as G
    G.install_shims()
    import daft_exprt.hparams as ref_hparams
    import daft_exprt.model as ref_model
    import daft_exprt.train as ref_train
    hp = G.make_hparams(ref_hparams)
    model = ref_model.DaftExprt(hp)
    params = list(model.parameters())
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(((torch.arange(p.numel()) % 251) / 256. + i / 8.).reshape(p.shape))
    opt = torch.optim.Adam(params, lr=1e-4, betas=hp.betas, eps=hp.epsilon, weight_decay=hp.weight_decay, amsgrad=False)
    for s in range(2):
        for i, p in enumerate(params):
            p.grad = (((torch.arange(p.numel()) * (s + 2)) % 7 - 3.) / 64. + i / 1024.).reshape(p.shape)
        opt.step()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'checkpoints', 'DaftExprt_2')
        ref_train.save_checkpoint(model, opt, hp, 3.3e-4, 2, best_val_loss=1.25, filepath=path)
        raw = open(path, 'rb').read()
    with open(OUT, 'wb') as f:
        f.write(lzma.compress(raw, preset=9 | lzma.PRESET_EXTREME))
    print(f'{OUT}: {len(raw)} bytes -> {os.path.getsize(OUT)} bytes, {len(model.state_dict())} tensors')


if __name__ == '__main__':
    main()
