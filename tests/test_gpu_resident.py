"""Batches collated on the device from a resident set (csrc/collate.hip, daft_exprt/resident_set.py) against the project's host
path: `DaftExprtDataCollate` -> (`group_host_batches`) -> `DaftExprt.parse_batch`.  Every comparison is bit-equal, dtypes and shapes
included.  The host collate's row order among equal phoneme counts is arbitrary (`torch.sort(descending=True)` is not stable), so
host rows are matched to device rows by (feature_dir, feature_file); that the device order is the stable descending one is asserted
separately.  Small shapes only."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from daft_exprt import config
from daft_exprt.data_loader import DaftExprtDataCollate, GroupedBatch, HostUnits, SyntheticUtterances, finish_group, \
    group_host_batches
from daft_exprt.model import DaftExprt
from daft_exprt.resident_set import GATHER_SPAN, ResidentBatch, ResidentLoader, ResidentSet, stable_order
from tests.util import make_hparams

DEV = 'cuda:0'
NAMES = ('symbols', 'durations_float', 'durations_int', 'symbols_energy', 'symbols_pitch', 'input_lengths', 'frames_energy',
         'frames_pitch', 'mel_specs', 'output_lengths', 'speaker_ids')


@pytest.fixture()
def poison():
    old = config.POISON
    config.POISON = True
    try:
        yield
    finally:
        config.POISON = old


def parse_host(hp, batch):
    ''' the project's `parse_batch` on a collate output, without building a model around it '''
    shim = SimpleNamespace(hp=hp)
    shim.check_ids = lambda *a, **k: DaftExprt.check_ids(shim, *a, **k)
    return DaftExprt.parse_batch(shim, torch.device(DEV), batch)


def utterance(hp, k, L, T):
    ''' one `SyntheticUtterances` item of exactly L symbols and T frames, under a name of its own '''
    item = SyntheticUtterances(hp, 1, seed=100 + k, t_min=T, t_max=T, l_range=(L, L), force_first_full=False)[0]
    assert len(item[0]) == L and item[7].shape == (hp.n_mel_channels, T)
    item[10] = f'utt{k:03d}_L{L}_T{T}'
    return item


def match_rows(host_keys, dev_keys):
    ''' for every host row, a device row holding the same utterance (each device row used once) '''
    free = {}
    for r, key in enumerate(dev_keys):
        free.setdefault(key, []).append(r)
    return [free[key].pop(0) for key in host_keys]


def assert_same_inputs(dev_inputs, host_inputs, rows, lo=0):
    for name, d, h in zip(NAMES, dev_inputs, host_inputs):
        d = d[lo:lo + len(rows)][rows] if rows is not None else d
        assert d.dtype == h.dtype and d.shape == h.shape and d.device == h.device, (name, d.dtype, h.dtype, d.shape, h.shape)
        assert torch.equal(d, h) and bool(torch.isfinite(d).all()), name


def check_batch(hp, items, batch):
    ''' `batch` = the device collate of `items` (in the sampler's order) against the host collate + parse_batch '''
    assert isinstance(batch, ResidentBatch) and isinstance(batch, tuple) and len(batch) == 13
    host_inputs, _, (h_dirs, h_files) = parse_host(hp, DaftExprtDataCollate(hp)(items))
    rows = match_rows(list(zip(h_dirs, h_files)), list(zip(batch[11], batch[12])))
    assert sorted(rows) == list(range(len(items)))
    for t in batch[:11]:
        assert t.is_contiguous()
    assert_same_inputs(batch[:11], host_inputs, rows)
    # the order: stable, descending, and the host's statement of it equals what the kernel wrote
    L = [len(it[0]) for it in items]
    want = stable_order(L).tolist()
    assert batch.order == want == batch.device_order.tolist()
    assert batch[5].tolist() == [L[p] for p in want] and batch[9].tolist() == [items[p][7].shape[1] for p in want]
    assert batch[12] == [items[p][10] for p in want] and batch[11] == [items[p][9] for p in want]
    assert batch.frames == sum(it[7].shape[1] for it in items) and isinstance(batch.frames, int)


def golden_hparams(golden_dir, **kw):
    fx = np.load(os.path.join(golden_dir, 'data_loader.npz'))
    hp = make_hparams(training_files=os.path.join(golden_dir, 'train_list.txt'), validation_files=os.path.join(golden_dir, 'train_list.txt'),
                      **kw)
    hp.stats = {f'spk {i}': {'energy': {'mean': float(fx['stats_energy_mean'][i]), 'std': float(fx['stats_energy_std'][i])},
                             'pitch': {'mean': float(fx['stats_pitch_mean'][i]), 'std': float(fx['stats_pitch_std'][i])}} for i in range(11)}
    return hp


def test_golden_set_as_one_batch(golden_dir):
    hp = golden_hparams(golden_dir)
    cwd = os.getcwd()
    os.chdir(golden_dir)
    try:
        rs = ResidentSet.from_list(hp.training_files, hp, DEV)
        from daft_exprt.data_loader import DaftExprtDataLoader
        ds = DaftExprtDataLoader(hp.training_files, hp)
        items = [ds[i] for i in range(len(ds))]
    finally:
        os.chdir(cwd)
    batches = list(ResidentLoader(rs, len(rs), shuffle=False, drop_last=False))
    assert len(batches) == 1 and batches[0][8].shape == (5, 80, 30)
    check_batch(hp, items, batches[0])


SPAN = GATHER_SPAN
# name -> ([(L, T) of every utterance of the store], the batch as positions in the store)
CASES = {
    'B1': ([(5, 9), (7, 12), (4, 6)], [1]),
    'equal_L_is_stable': ([(5, 9), (5, 14), (5, 3), (5, 11)], [2, 0, 3]),
    'L1_and_T1': ([(1, 7), (2, 1), (6, 10)], [0, 1, 2]),
    'first_and_last_of_the_store': ([(4, 6), (7, 12), (3, 5), (8, 8), (5, 9), (6, 13)], [5, 2, 0]),
    'same_index_twice': ([(4, 6), (7, 12), (3, 5)], [2, 2, 1]),
    'odd_T_throughout': ([(4, 7), (7, 13), (3, 5), (8, 9), (5, 21)], [0, 1, 2, 3, 4]),
    'T_pad_one_below_the_span': ([(4, 7), (9, SPAN - 1), (3, 5)], [0, 1, 2]),
    'T_pad_equal_to_the_span': ([(4, 7), (9, SPAN), (3, 5)], [0, 1, 2]),
    'T_pad_one_above_the_span': ([(4, 7), (SPAN + 1, SPAN + 1), (3, 5)], [0, 1, 2]),      # (L_pad crosses it too)
}


@pytest.mark.parametrize('case', list(CASES))
def test_edge_cases_under_poison(case, poison):
    hp = make_hparams()
    shapes, picks = CASES[case]
    store = [utterance(hp, k, L, T) for k, (L, T) in enumerate(shapes)]
    loader = ResidentLoader(ResidentSet.from_items(store, hp, DEV), len(picks))
    check_batch(hp, [store[i] for i in picks], loader.collate([picks]))


def test_more_rows_than_one_workgroups_lanes(poison):
    hp = make_hparams()
    ds = SyntheticUtterances(hp, 48, seed=21, t_max=64, l_range=(3, 20), force_first_full=False)
    store = [ds[i] for i in range(48)]
    assert max(it[7].shape[1] for it in store) <= 64 and len({len(it[0]) for it in store}) < 48      # (ties among the 48)
    picks = torch.randperm(48, generator=torch.Generator().manual_seed(3)).tolist()
    loader = ResidentLoader(ResidentSet.from_items(store, hp, DEV), 48)
    check_batch(hp, [store[i] for i in picks], loader.collate([picks]))


GROUP_SHAPES = [(5, 9), (3, 14), (8, 21), (8, 6), (2, 31), (4, 17)]      # 3 x 2: (L_pad, T_pad) = (5, 14), (8, 21), (4, 31)
# max(0, min(length, pad - 2)) of each of the six, worked out by hand
GROUP_SKIP_IN, GROUP_SKIP_OUT = [3, 3, 6, 6, 2, 2], [9, 12, 19, 6, 29, 17]


def group_rows(h_dirs, h_files, g):
    ''' `match_rows` per micro-batch of 2: for every host row of the group, the device row of `g` with the same utterance '''
    rows = []
    for k in range(3):
        sl = slice(2 * k, 2 * k + 2)
        rows += [2 * k + r for r in match_rows(list(zip(h_dirs[sl], h_files[sl])), list(zip(g.dirs[sl], g.files[sl])))]
    assert sorted(rows) == list(range(6))
    return rows


def assert_same_bounds(dev_bounds, host_bounds, rows):
    assert len(dev_bounds) == len(host_bounds) == 4
    for name, d, h in zip(('skip_in', 'nmax_in', 'skip_out', 'nmax_out'), dev_bounds, host_bounds):
        assert d.dtype == h.dtype == torch.int64 and d.shape == h.shape and torch.equal(d[rows], h), name


def test_grouped_micro_batches(poison):
    hp = make_hparams()
    shapes = GROUP_SHAPES
    store = [utterance(hp, k, L, T) for k, (L, T) in enumerate(shapes)]
    units = list(ResidentLoader(ResidentSet.from_items(store, hp, DEV), 2, shuffle=False, drop_last=True, group=3))
    assert len(units) == 1
    g = units[0]
    assert isinstance(g, GroupedBatch) and g.accum == 3 and g.sizes == [2, 2, 2]
    host = [DaftExprtDataCollate(hp)(store[2 * k:2 * k + 2]) for k in range(3)]
    merged, nmax, sizes = group_host_batches(host)
    assert sizes == g.sizes and len(sizes) == g.accum
    inputs, targets, (h_dirs, h_files) = parse_host(hp, merged)
    h = finish_group(inputs, targets, nmax, sizes)      # the host path's own finish of the group on the device
    assert isinstance(h, GroupedBatch) and h.inputs is inputs and h.targets is targets and h.accum == 3 and h.sizes == sizes
    skip_in, nmax_in, skip_out, nmax_out = h.bounds
    assert nmax_in.tolist() == [5, 5, 8, 8, 4, 4] and nmax_out.tolist() == [14, 14, 21, 21, 31, 31]
    rows = group_rows(h_dirs, h_files, g)
    assert_same_inputs(g.inputs, inputs, rows)
    assert g[0] is g.inputs and g[1] is g.targets and len(g.bounds) == 4
    assert_same_bounds(g.bounds, h.bounds, rows)
    for t, k in zip(g.targets, (1, 3, 4, 8, 10)):      # the views parse_batch hands out
        assert t is g.inputs[k]
    want = [int(p) for k in range(3) for p in stable_order([len(it[0]) for it in store[2 * k:2 * k + 2]])]
    assert g.order == want == g.device_order.tolist() and g.frames == sum(T for _, T in shapes)
    # both paths against the hand-made values: device row r of micro-batch k holds utterance 2 k + order[r] of the store
    utt = [2 * (r // 2) + p for r, p in enumerate(g.order)]
    assert g.bounds[0].tolist() == [GROUP_SKIP_IN[u] for u in utt] and g.bounds[2].tolist() == [GROUP_SKIP_OUT[u] for u in utt]
    assert skip_in.tolist() == [GROUP_SKIP_IN[utt[r]] for r in rows] and skip_out.tolist() == [GROUP_SKIP_OUT[utt[r]] for r in rows]


def test_host_and_resident_feeders_yield_the_same_units(poison):
    ''' `HostUnits` over a DataLoader and `ResidentLoader`, as the train loop drives them, over the same six utterances '''
    hp = make_hparams()
    store = [utterance(hp, k, L, T) for k, (L, T) in enumerate(GROUP_SHAPES)]
    names = []
    model = SimpleNamespace(parse_batch=lambda gpu, batch: (names.append((batch[11], batch[12])), parse_host(hp, batch))[1])
    loader = torch.utils.data.DataLoader(store, batch_size=2, shuffle=False, drop_last=True, collate_fn=DaftExprtDataCollate(hp))
    host_units = list(HostUnits(loader, 3).units(model, DEV))
    resident = ResidentLoader(ResidentSet.from_items(store, hp, DEV), 2, shuffle=False, drop_last=True, group=3)
    resident_units = list(resident.units(model, DEV))
    assert len(host_units) == len(resident_units) == len(names) == 1 and resident.held == []
    (h, h_frames), (g, g_frames) = host_units[0], resident_units[0]
    assert isinstance(h, GroupedBatch) and isinstance(g, GroupedBatch) and h.accum == g.accum == 3 and h.sizes == g.sizes == [2, 2, 2]
    rows = group_rows(*names[0], g)
    assert_same_inputs(g.inputs, h.inputs, rows)
    assert_same_bounds(g.bounds, h.bounds, rows)
    assert h_frames == g_frames == sum(T for _, T in GROUP_SHAPES) and isinstance(h_frames, int) and isinstance(g_frames, int)


def test_batches_do_not_depend_on_what_ran_before():
    hp = make_hparams()
    ds = SyntheticUtterances(hp, 9, seed=33, t_max=40, l_range=(3, 9), force_first_full=False)
    store = [ds[i] for i in range(9)]
    rs = ResidentSet.from_items(store, hp, DEV)

    def two_epochs():
        torch.manual_seed(5)
        loader = ResidentLoader(rs, 2, shuffle=True, drop_last=True)
        lists, batches = [], []
        for _ in range(2):
            lists.append(loader.index_lists())
        torch.manual_seed(5)
        for _ in range(2):
            batches += list(loader)
        return lists, batches
    (lists_a, run_a), (lists_b, run_b) = two_epochs(), two_epochs()
    assert lists_a == lists_b and len(run_a) == len(run_b) == 8 and lists_a[0] != lists_a[1]
    flat = [b for epoch in lists_a for b in epoch]
    for idx, a, b in zip(flat, run_a, run_b):
        assert sorted(a[12]) == sorted(store[i][10] for i in idx)      # the loader ran the lists it reported
        assert a[12] == b[12] and all(torch.equal(x, y) for x, y in zip(a[:11], b[:11]))
    # a batch produced after another batch equals the same batch produced first
    loader = ResidentLoader(rs, 3)
    first = loader.collate([[4, 1, 7]])
    loader.collate([[0, 8, 2]])
    again = ResidentLoader(rs, 3).collate([[0, 8, 2]])
    later = loader.collate([[4, 1, 7]])
    after = loader.collate([[0, 8, 2]])
    for x, y in zip(first[:11], later[:11]):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    for x, y in zip(again[:11], after[:11]):
        assert torch.equal(x, y)
    check_batch(hp, [store[i] for i in (0, 8, 2)], after)


def run_train(golden_dir, out, resident, ddp_flag, port):
    from daft_exprt.train import train
    hp = golden_hparams(golden_dir, output_directory=out, batch_size=2, accumulation_steps=2, nb_iterations=2, iters_per_checkpoint=2,
                        iters_check_for_model_improvement=1, resident_data_set=resident)
    hp.rank, hp.world_size, hp.multiprocessing_distributed = 0, 1, ddp_flag
    hp.ngpus_per_node, hp.dist_url = 1, f'tcp://127.0.0.1:{port}'
    cwd = os.getcwd()
    os.chdir(golden_dir)
    try:
        os.makedirs(os.path.join(out, 'logs'), exist_ok=True)
        train(0, hp, os.path.join(out, 'logs', 'train.log'))
    finally:
        os.chdir(cwd)
    assert not torch.distributed.is_initialized()
    recs = [json.loads(l) for l in open(os.path.join(out, 'logs', 'metrics.jsonl'))]
    return hp, [r for r in recs if 'DaftExprt.training/loss' in r], [r for r in recs if 'DaftExprt.validation/loss' in r]


@pytest.fixture(scope='module')
def loader_path_frames(golden_dir, tmp_path_factory):
    ''' `valid_frames` per iteration of the unchanged DataLoader path with the distributed flag on (a deterministic sampler) '''
    _, recs, _ = run_train(golden_dir, str(tmp_path_factory.mktemp('loader_path')), False, True, 29541)
    return [r['valid_frames'] for r in recs]


@pytest.mark.parametrize('ddp_flag', [True, False])
def test_train_from_a_resident_set(golden_dir, tmp_path, ddp_flag, loader_path_frames, monkeypatch):
    from daft_exprt import resident_set
    made = []

    def spy(*args, **kw):
        made.append(prepare(*args, **kw))
        return made[-1]
    prepare = resident_set.prepare_resident_loaders
    monkeypatch.setattr(resident_set, 'prepare_resident_loaders', spy)
    out = str(tmp_path)
    hp, recs, vals = run_train(golden_dir, out, True, ddp_flag, 29542 if ddp_flag else 29543)
    # train() ran on the resident loaders: grouped micro-batches, the launches on its copy stream, the sampler of the launch mode
    (train_loader, sampler, val_loader, n), = made
    assert isinstance(train_loader, ResidentLoader) and isinstance(val_loader, ResidentLoader) and n == 5
    assert train_loader.group == 2 and train_loader.stream is not None and val_loader.stream is None and (sampler is not None) == ddp_flag
    assert [r['iteration'] for r in recs] == [1, 2] and [r['iteration'] for r in vals] == [1, 2]
    assert all(math.isfinite(r['DaftExprt.training/loss']) and r['DaftExprt.optimization/grad_norm'] > 0 for r in recs)
    assert all(math.isfinite(r['DaftExprt.validation/loss']) for r in vals)
    assert all(isinstance(r['valid_frames'], int) and r['valid_frames'] > 0 for r in recs)
    if ddp_flag:      # DistributedSampler(shuffle=False): the same utterances in the same batches on both paths
        assert [r['valid_frames'] for r in recs] == loader_path_frames
    for name, it in (('DaftExprt_best', None), ('DaftExprt_2', 2)):
        ckpt = torch.load(os.path.join(out, 'checkpoints', name), weights_only=False)
        assert len(ckpt['state_dict']) == 193 and (it is None or ckpt['iteration'] == it)
        assert all(k.startswith('module.') == ddp_flag for k in ckpt['state_dict'])
        model = DaftExprt(hp)
        model.load_state_dict({k.replace('module.', ''): v for k, v in ckpt['state_dict'].items()})
