"""Checkpoint interop with the reference's own `save_checkpoint` / `load_checkpoint` (train.py:56-136) and `torch.optim.Adam` state,
in both directions, at the full default architecture (193 tensors, 14.7 M parameters), against tests/golden/ref_checkpoint.xz: a
file the reference's `save_checkpoint` wrote after two `torch.optim.Adam` steps (tools/gen_golden_checkpoint.py).

  1. this package's `load_checkpoint` reads that file into `DaftExprt` + `FusedAdam`: every tensor, both Adam moments of each, the
     step count, iteration / learning rate / best validation loss must come back bit for bit;
  2. the way back: what this package's `save_checkpoint` writes must be what the reference's `load_checkpoint` consumes -- the same
     top-level entries, feature hyper-parameters equal, a `state_dict` that loads strictly into a module with the reference's
     parameter names, order and shapes, and an optimizer state that a `torch.optim.Adam` over those parameters takes with the
     reference trainer's settings -- with the values of the reference-written file.
tools/ref_checkpoint_roundtrip.py runs the same round trip through the reference's code itself where it is available."""
import lzma
import os

import torch

from daft_exprt import train as T
from daft_exprt.model import DaftExprt
from daft_exprt.optim import FusedAdam
from tests.util import make_hparams


def _load_golden(golden_dir, tmp_path):
    path = tmp_path / 'checkpoints' / 'DaftExprt_2'
    path.parent.mkdir()
    with lzma.open(os.path.join(golden_dir, 'ref_checkpoint.xz')) as f:
        path.write_bytes(f.read())
    return str(path), torch.load(str(path), map_location='cpu', weights_only=False)


def _reference_shaped_module(state_dict):
    ''' a module whose parameters carry the reference model's names, order and shapes (what its strict `load_state_dict` checks) '''
    root = torch.nn.Module()
    for name, t in state_dict.items():
        node, parts = root, name.split('.')
        for part in parts[:-1]:
            if not hasattr(node, part):
                setattr(node, part, torch.nn.Module())
            node = getattr(node, part)
        setattr(node, parts[-1], torch.nn.Parameter(torch.zeros_like(t)))
    return root


def test_reference_written_checkpoint_loads_and_ours_loads_in_the_reference(golden_dir, tmp_path):
    path, ref = _load_golden(golden_dir, tmp_path)
    ref_state, ref_opt = ref['state_dict'], ref['optimizer']
    assert len(ref_state) == 193 and len(ref_opt['state']) == 193

    # ---- the reference's file, read by this package
    hp = make_hparams(output_directory=str(tmp_path))
    torch.manual_seed(99)                                  # different initial weights: everything must come from the file
    model = DaftExprt(hp)
    opt = FusedAdam(model, betas=hp.betas, eps=hp.epsilon, weight_decay=hp.weight_decay)
    model, opt, iteration, lr, best = T.load_checkpoint(path, 0, model, opt, hp)
    assert (iteration, lr, best) == (2, 3.3e-4, 1.25), (iteration, lr, best)
    sd = model.state_dict()
    assert list(sd.keys()) == list(ref_state.keys())
    for k in sd:
        assert sd[k].dtype == ref_state[k].dtype and torch.equal(sd[k].cpu(), ref_state[k]), k
    assert opt.step_count == 2
    mine_opt = opt.state_dict()
    assert len(mine_opt['state']) == 193
    for idx, st in ref_opt['state'].items():
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(mine_opt['state'][idx][key].cpu(), st[key]), (idx, key)
        assert float(mine_opt['state'][idx]['step']) == float(st['step']) == 2.
    for key in ('lr', 'betas', 'eps', 'weight_decay', 'amsgrad'):
        assert tuple(mine_opt['param_groups'][0][key]) == tuple(ref_opt['param_groups'][0][key]) if key == 'betas' else \
            mine_opt['param_groups'][0][key] == ref_opt['param_groups'][0][key], key

    # ---- the way back: this package's file, consumed the way the reference's load_checkpoint does
    back = str(tmp_path / 'checkpoints' / 'DaftExprt_back')
    T.save_checkpoint(model, opt, hp, 4.4e-4, 7, best_val_loss=0.5, filepath=back)
    mine = torch.load(back, map_location='cpu', weights_only=False)
    assert set(mine) == set(ref)
    assert (mine['iteration'], mine['learning_rate'], mine['best_val_loss']) == (7, 4.4e-4, 0.5)
    for key in T.FEATURES_HPARAMS:
        assert mine['config_params'][key] == ref['config_params'][key], key
    stand_in = _reference_shaped_module(ref_state)
    stand_in.load_state_dict(mine['state_dict'], strict=True)
    for k, v in stand_in.state_dict().items():
        assert v.dtype == ref_state[k].dtype and torch.equal(v, ref_state[k]), k
    params = list(stand_in.parameters())
    adam = torch.optim.Adam(params, lr=1e-4, betas=hp.betas, eps=hp.epsilon, weight_decay=hp.weight_decay)
    adam.load_state_dict(mine['optimizer'])
    st2 = adam.state_dict()['state']
    for idx, st in ref_opt['state'].items():
        assert torch.equal(st2[idx]['exp_avg'], st['exp_avg']) and torch.equal(st2[idx]['exp_avg_sq'], st['exp_avg_sq']), idx
        assert float(st2[idx]['step']) == 2.
    assert adam.param_groups[0]['lr'] == ref_opt['param_groups'][0]['lr']
