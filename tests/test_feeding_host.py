"""Host side of what feeds the train loop (`data_loader`: `group_bounds`, `take_groups`, `check_group_sizes`, `HostUnits`; the same
rules inside `resident_set.ResidentLoader`; `train.step_record`).  No GPU: nothing here reaches a launch."""
import pytest
import torch

from daft_exprt.data_loader import HostUnits, SyntheticUtterances, group_bounds, group_host_batches, group_micro_batches, \
    synthetic_batch, take_groups
from daft_exprt.resident_set import ResidentLoader, ResidentSet
from daft_exprt.train import step_record
from tests.util import make_hparams

# 5 batches an epoch, groups of 2: (groups, held) of the first and of the second epoch, in batch numbers
EPOCH_1 = ([[0, 1], [2, 3]], [4])
EPOCH_2 = ([[4, 0], [1, 2], [3, 4]], [])
RAGGED = r'micro-batches of different sizes \[2, 1\]: set hparams.group_micro_batches = False'


def resident_set(n):
    hp = make_hparams()
    ds = SyntheticUtterances(hp, n, seed=7, t_max=24, l_range=(3, 8), force_first_full=False)
    return ResidentSet.from_items([ds[i] for i in range(n)], hp, 'cpu')


def test_carry_over_is_one_rule_for_both_feeders():
    assert take_groups([], list(range(5)), 2) == EPOCH_1
    assert take_groups(EPOCH_1[1], list(range(5)), 2) == EPOCH_2
    assert take_groups([], [0, 1], 3) == ([], [0, 1]) and take_groups([7], [8, 9], 1) == ([[7], [8], [9]], [])
    # the resident loader: 10 utterances in batches of 2 = the same 5 batches an epoch, as index lists
    loader = ResidentLoader(resident_set(10), 2, shuffle=False, drop_last=True, group=2)
    number = lambda plan: [[b[0] // 2 for b in unit] for unit in plan]
    for groups, held in (EPOCH_1, EPOCH_2):
        assert number(loader.plan_epoch()) == groups and number([loader.held]) == [held]
    # the host path: 5 collate outputs of 2 utterances each, every one with pads of its own
    hp = make_hparams()
    batches = [synthetic_batch(hp, 2, seed=40 + k, t_max=31 - 3 * k, l_range=(3, 8 - k), force_first_full=True) for k in range(5)]
    assert all(b[0].shape[1] <= 8 and b[8].shape[2] <= 31 for b in batches) and len({b[8].shape[2] for b in batches}) == 5
    feeder = HostUnits(batches, 2)
    for groups, held in (EPOCH_1, EPOCH_2):
        units = list(feeder.plan())
        assert len(units) == len(groups)
        for (merged, (nmax, sizes)), members in zip(units, groups):
            want, want_nmax, want_sizes = group_host_batches([batches[k] for k in members])
            assert len(merged) == 13 and all(torch.equal(x, y) for x, y in zip(merged[:11], want[:11]))
            assert merged[11] == want[11] and merged[12] == want[12] and sizes == want_sizes == [2, 2]
            assert all(torch.equal(x, y) for x, y in zip(nmax, want_nmax))
        assert len(feeder.held) == len(held) and all(x is batches[k] for x, k in zip(feeder.held, held))
    # without a group every batch is a unit of its own and nothing is held
    feeder = HostUnits(batches, 1)
    assert [(b is x, g) for (b, g), x in zip(feeder.plan(), batches)] == [(True, None)] * 5 and feeder.held == []


def test_a_ragged_group_is_refused_where_either_feeder_plans_it():
    hp = make_hparams()
    batches = [synthetic_batch(hp, n, seed=50 + n, t_max=20, l_range=(3, 8), force_first_full=False) for n in (2, 1)]
    with pytest.raises(AssertionError, match=RAGGED):
        next(HostUnits(batches, 2).plan())
    loader = ResidentLoader(resident_set(3), 2, shuffle=False, drop_last=False, group=2)       # batches [0 1] [2]
    with pytest.raises(AssertionError, match=RAGGED):
        next(iter(loader))


def test_group_bounds_is_the_clamp():
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    bounds = group_bounds(t(5, 1, 0, 9), t(5, 5, 8, 8), t(5, 1, 0, 9), t(5, 5, 8, 8))
    assert [b.tolist() for b in bounds] == [[3, 1, 0, 6], [5, 5, 8, 8]] * 2 and all(b.dtype == torch.int64 for b in bounds)

    def batch(in_len, L, out_len, T):      # an 11-tuple of inputs in `parse_batch` order, two utterances
        sym, frm = torch.zeros(2, L), torch.zeros(2, T)
        return (sym.long(), sym, sym.long(), sym, sym, t(*in_len), frm, frm, torch.zeros(2, 80, T), t(*out_len), t(0, 1)), None
    g = group_micro_batches([batch((5, 1), 5, (9, 4), 9), batch((8, 3), 8, (14, 2), 14)])
    want = group_bounds(t(5, 1, 8, 3), t(5, 5, 8, 8), t(9, 4, 14, 2), t(9, 9, 14, 14))
    assert [b.tolist() for b in want] == [[3, 1, 6, 3], [5, 5, 8, 8], [7, 4, 12, 2], [9, 9, 14, 14]]
    assert len(g.bounds) == 4 and all(x.dtype == torch.int64 and torch.equal(x, y) for x, y in zip(g.bounds, want))


def test_step_record_is_the_line_train_writes():
    values = [0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 15.875, 3.5]
    assert step_record(7, 1e-4, 0.75, 1234, values) == {
        'iteration': 7, 'DaftExprt.optimization/grad_norm': 3.5, 'DaftExprt.optimization/learning_rate': 1e-4,
        'DaftExprt.optimization/duration': 0.75, 'DaftExprt.training/loss': 15.875, 'valid_frames': 1234,
        'DaftExprt.training/speaker_loss': 0.125, 'DaftExprt.training/post_mult_loss': 0.25, 'DaftExprt.training/duration_loss': 0.5,
        'DaftExprt.training/energy_loss': 1.0, 'DaftExprt.training/pitch_loss': 2.0, 'DaftExprt.training/mel_spec_l1_loss': 4.0,
        'DaftExprt.training/mel_spec_l2_loss': 8.0}
    assert list(step_record(7, 1e-4, 0.75, 1234, values))[:6] == [
        'iteration', 'DaftExprt.optimization/grad_norm', 'DaftExprt.optimization/learning_rate', 'DaftExprt.optimization/duration',
        'DaftExprt.training/loss', 'valid_frames']
