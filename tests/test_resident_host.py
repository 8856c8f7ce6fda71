"""Host side of the resident training set (daft_exprt/resident_set.py, csrc/collate.hip): packing, the stable order rule, batch
composition against torch's own samplers, the group carry-over, the memory fallback and the new entry points' argument checks.
No GPU: the sets are packed on the CPU and nothing is launched."""
import contextlib
import os

import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, DataLoader, RandomSampler, SequentialSampler
from torch.utils.data.distributed import DistributedSampler

from daft_exprt import _hip as H
from daft_exprt.data_loader import DaftExprtDataLoader, SyntheticUtterances
from daft_exprt.resident_set import GATHER_SPAN, MAX_BATCH, ResidentLoader, ResidentSet, list_bytes, prepare_resident_loaders, \
    stable_order
from tests.util import make_hparams


def golden_hparams(golden_dir, **kw):
    fx = np.load(os.path.join(golden_dir, 'data_loader.npz'))
    hp = make_hparams(training_files=os.path.join(golden_dir, 'train_list.txt'), validation_files=os.path.join(golden_dir, 'train_list.txt'),
                      **kw)
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    return hp, fx


@contextlib.contextmanager
def inside(path):
    ''' the golden list names its feature directories relative to tests/golden '''
    cwd = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(cwd)


def small_set(n=5, **kw):
    hp = make_hparams()
    ds = SyntheticUtterances(hp, n, seed=7, t_max=24, l_range=(3, 8), force_first_full=False)
    return ResidentSet.from_items([ds[i] for i in range(n)], hp, 'cpu', **kw), hp


def test_packing_keeps_the_loaders_shuffle_order(golden_dir):
    hp, fx = golden_hparams(golden_dir)
    with inside(golden_dir):
        rs = ResidentSet.from_list(hp.training_files, hp, 'cpu')
    assert len(rs) == int(fx['n_items']) and rs.n_global == len(rs)
    assert rs.files == [str(fx[f'item{i}_file']) for i in range(len(rs))]
    assert rs.speaker.tolist() == [int(fx[f'item{i}_speaker']) for i in range(len(rs))]


def test_offsets_reproduce_every_items_arrays(golden_dir):
    hp, _ = golden_hparams(golden_dir)
    with inside(golden_dir):
        rs = ResidentSet.from_list(hp.training_files, hp, 'cpu')
        ds = DaftExprtDataLoader(hp.training_files, hp)
        items = [ds[i] for i in range(len(ds))]
        assert rs.nbytes == list_bytes(hp.training_files, hp)
    assert rs.sym_off.dtype == rs.frm_off.dtype == rs.speaker.dtype == torch.int64
    assert rs.sym_off.tolist() == np.concatenate(([0], np.cumsum([len(it[0]) for it in items]))).tolist()
    assert rs.frm_off.tolist() == np.concatenate(([0], np.cumsum([it[7].shape[1] for it in items]))).tolist()
    assert rs.mel.numel() == hp.n_mel_channels * int(rs.frm_off[-1]) and rs.mel.dtype == torch.float32
    assert rs.L.tolist() == [len(it[0]) for it in items] and rs.T.tolist() == [it[7].shape[1] for it in items]
    for u, want in enumerate(items):
        got = rs.item(u)
        for k in range(8):
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k].to(got[k].dtype)), (u, k)
            assert torch.equal(got[k].to(want[k].dtype), want[k]), (u, k)
        assert tuple(got[8:]) == tuple(want[8:])
    # a shard: only the utterances asked for, numbered as the whole list numbers them
    with inside(golden_dir):
        shard = ResidentSet.from_list(hp.training_files, hp, 'cpu', indices=[3, 0])
    assert shard.files == [rs.files[3], rs.files[0]] and shard.index.tolist() == [3, 0] and shard.n_global == len(rs)
    assert torch.equal(shard.item(0)[7], rs.item(3)[7]) and torch.equal(shard.item(1)[0], rs.item(0)[0])


def test_packing_rejects_out_of_range_ids():
    hp = make_hparams()
    ds = SyntheticUtterances(hp, 3, seed=5, t_max=20, l_range=(3, 6), force_first_full=False)
    items = [ds[i] for i in range(3)]
    ResidentSet.from_items(items, hp, 'cpu')
    bad = [list(it) for it in items]
    bad[1][0] = bad[1][0].clone()
    bad[1][0][0] = hp.n_symbols
    with pytest.raises(IndexError, match='symbol id out of range'):
        ResidentSet.from_items(bad, hp, 'cpu')
    bad = [list(it) for it in items]
    bad[2][8] = hp.n_speakers - 1                 # the classifier has n_speakers - 1 targets
    with pytest.raises(IndexError, match='speaker id out of range'):
        ResidentSet.from_items(bad, hp, 'cpu')


def reference_rank(lengths):
    ''' the rule as the issue states it: entries with a larger L, plus earlier entries with an equal L '''
    order = [0] * len(lengths)
    for b, l in enumerate(lengths):
        order[sum(1 for x in lengths if x > l) + sum(1 for x in lengths[:b] if x == l)] = b
    return order


@pytest.mark.parametrize('lengths, want', [([7, 7, 7, 7], [0, 1, 2, 3]),                    # all equal: the sampler's order
                                           ([1, 2, 3, 4, 5], [4, 3, 2, 1, 0]),              # strictly increasing: reversed
                                           ([5, 9, 5, 2, 9, 5], [1, 4, 0, 2, 5, 3])])       # two tie groups
def test_stable_order(lengths, want):
    assert stable_order(lengths).tolist() == want == reference_rank(lengths)


@pytest.mark.parametrize('drop_last', [False, True])
def test_index_lists_are_the_torch_samplers(drop_last):
    rs, _ = small_set(5)
    loader = ResidentLoader(rs, 2, shuffle=False, drop_last=drop_last)
    want = [list(b) for b in BatchSampler(SequentialSampler(range(5)), 2, drop_last)]
    assert loader.index_lists() == want and len(loader) == len(want) == (2 if drop_last else 3)
    assert loader.plan_epoch() == [[b] for b in want]
    # two ranks over 5 items: DistributedSampler(shuffle=False) strides and pads by repeating the first item
    hp = make_hparams()
    ds = SyntheticUtterances(hp, 5, seed=7, t_max=24, l_range=(3, 8), force_first_full=False)
    seen = []
    for rank in range(2):
        sampler = DistributedSampler(range(5), num_replicas=2, rank=rank, shuffle=False)
        held = sorted(set(sampler))
        shard = ResidentSet.from_items([ds[i] for i in held], hp, 'cpu', index=held, n_global=5)
        loader = ResidentLoader(shard, 2, drop_last=drop_last, distributed=(2, rank))
        want = [list(b) for b in BatchSampler(sampler, 2, drop_last)]
        assert loader.index_lists() == want
        plan = loader.plan_epoch()                      # the same utterances through the shard's own numbering
        assert [[int(shard.index[u]) for u in mb] for unit in plan for mb in unit] == want
        seen.append([g for b in want for g in b] if not drop_last else None)
    if not drop_last:
        assert seen == [[0, 2, 4], [1, 3, 0]]


def test_shuffled_index_lists_follow_torchs_generator():
    rs, _ = small_set(5)
    loader = ResidentLoader(rs, 2, shuffle=True, drop_last=True)
    torch.manual_seed(11)
    a = [loader.index_lists(), loader.index_lists()]
    torch.manual_seed(11)
    b = [loader.index_lists(), loader.index_lists()]
    assert a == b and all(len(e) == 2 and len(set(i for bt in e for i in bt)) == 4 for e in a)
    torch.manual_seed(11)
    want = [list(bt) for bt in BatchSampler(RandomSampler(range(5)), 2, True)]
    assert a[0] == want                                 # torch's own RandomSampler under the same seed


def test_len_and_group_carry_over_across_the_epoch_boundary():
    rs, _ = small_set(5)
    loader = ResidentLoader(rs, 2, shuffle=False, drop_last=False, group=2)       # 3 batches an epoch: [0 1] [2 3] [4]
    assert len(loader) == 1
    assert loader.plan_epoch() == [[[0, 1], [2, 3]]] and loader.held == [[4]]
    assert len(loader) == 2                                                       # the carried batch counts
    assert loader.plan_epoch() == [[[4], [0, 1]], [[2, 3], [4]]] and loader.held == []
    assert len(loader) == 1
    # drop_last: 2 batches an epoch, nothing is carried
    loader = ResidentLoader(rs, 2, shuffle=False, drop_last=True, group=2)
    assert len(loader) == 1 and loader.plan_epoch() == [[[0, 1], [2, 3]]] and loader.held == [] and len(loader) == 1
    # accum 3 over 2 batches an epoch: the group closes in the second epoch
    loader = ResidentLoader(rs, 2, shuffle=False, drop_last=True, group=3)
    assert len(loader) == 0 and loader.plan_epoch() == [] and len(loader) == 1
    assert loader.plan_epoch() == [[[0, 1], [2, 3], [0, 1]]] and loader.held == [[2, 3]]


def test_a_set_above_the_memory_limit_gets_the_dataloaders(golden_dir, caplog):
    hp, _ = golden_hparams(golden_dir, batch_size=2)
    assert hp.resident_max_bytes == 32 * 1024 ** 3 and hp.resident_data_set is False
    with inside(golden_dir):
        hp.resident_max_bytes = list_bytes(hp.training_files, hp) * 2 - 1
        with caplog.at_level('WARNING', logger='daft_exprt.resident_set'):
            train_loader, sampler, val_loader, n = prepare_resident_loaders(hp, 'cpu', distributed=False)
        assert type(train_loader) is DataLoader and type(val_loader) is DataLoader and sampler is None and n == 5
        assert len([r for r in caplog.records if 'resident_max_bytes' in r.getMessage()]) == 1
        hp.resident_max_bytes += 1                      # exactly the packed size of both sets: resident
        train_loader, sampler, val_loader, n = prepare_resident_loaders(hp, 'cpu', distributed=False, group=2)
    assert isinstance(train_loader, ResidentLoader) and isinstance(val_loader, ResidentLoader) and sampler is None and n == 5
    assert train_loader.drop_last and train_loader.group == 2 and len(train_loader) == 1
    assert not val_loader.drop_last and val_loader.group == 1 and len(val_loader) == 3
    assert val_loader.index_lists() == [[0, 1], [2, 3], [4]]


def test_new_entry_points_check_their_arguments():
    lib = H.lib()
    names = {name for name, _, _ in H.header_prototypes()}
    for name in ('dx_collate_order', 'dx_collate_gather', 'dx_collate_max_batch', 'dx_collate_span'):
        assert name in names and hasattr(lib, name)
    assert lib.dx_abi_version() == 13
    assert MAX_BATCH == lib.dx_collate_max_batch() >= 256 and GATHER_SPAN == lib.dx_collate_span() > 0
    p = 8       # any non-null address: every check below answers before a launch
    assert lib.dx_collate_order(None, p, p, p, 4, p, p, p, p, p, p, None, None, None, None, 1, 2, None) == -1
    assert b'null' in lib.dx_last_error()
    assert lib.dx_collate_order(p, p, p, p, 4, p, p, p, p, p, p, p, None, p, p, 1, 2, None) == -1          # three of the four bounds
    assert lib.dx_collate_order(p, p, p, p, 4, p, p, p, p, p, p, None, None, None, None, 1, MAX_BATCH + 1, None) == -5
    assert b'LDS' in lib.dx_last_error()
    assert lib.dx_collate_order(p, p, p, p, 4, p, p, p, p, p, p, None, None, None, None, 0, 2, None) == -2
    assert lib.dx_collate_gather(p, p, p, 4, *([p] * 15), None, 2, 3, 4, 80, None) == -1
    assert b'null' in lib.dx_last_error()
    assert lib.dx_collate_gather(p, p, p, 4, *([p] * 16), 2, 0, 4, 80, None) == -2
    assert lib.dx_collate_gather(p, p, p, 4, *([p] * 16), 65536, 3, 4, 80, None) == -5
