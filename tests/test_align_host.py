"""Host side of the synthesis-based alignment (daft_exprt/align.py): the integer oracle of `dx_dtw_transfer` / `dx_active_span`
(tests/align_oracle.py) on hand-built paths whose answers are worked out in its comments, and `markers_from_durations`: the rows
it writes, that `extract_features.update_markers` reads them back as the phonemised sentence, and that the reference's frame
quantiser gives every written row frames again."""
import logging
import re

import numpy as np
import pytest

from oracle import daft_exprt_cpu as REF
from tests import align_oracle as A
from tests.util import make_hparams

ROW = re.compile(r'^\d+\.\d{6}\t\d+\.\d{6}\t\S+\t\S+\t\d+\n$')


@pytest.mark.parametrize('case', A.transfer_cases(), ids=lambda c: c[0])
def test_oracle_on_hand_built_paths(case):
    name, path, n_ref, n_gen, durations, min_frames, want = case
    got = A.dtw_transfer(path, n_ref, n_gen, durations, min_frames)
    assert got == want, (name, got, want)
    rec, moved, status = got
    if status == 0:
        assert sum(rec) == n_ref and all((r >= min_frames) if d > 0 else (r == 0) for r, d in zip(rec, durations))
    else:
        assert not any(rec) and moved == 0


def _monotone_path(n_ref, n_gen, rng):
    i = j = 0
    cells = [(0, 0)]
    while (i, j) != (n_ref - 1, n_gen - 1):
        moves = [m for m in ((1, 1), (1, 0), (0, 1)) if i + m[0] < n_ref and j + m[1] < n_gen]
        di, dj = moves[rng.randint(len(moves))]
        i, j = i + di, j + dj
        cells.append((i, j))
    return cells


def test_oracle_invariants_on_random_monotone_paths():
    rng = np.random.RandomState(3)
    seen = set()
    for _ in range(300):
        durations = rng.randint(0, 5, size=rng.randint(1, 12)).tolist()
        n_gen, n_ref, m = sum(durations), int(rng.randint(1, 40)), int(rng.randint(1, 4))
        if n_gen == 0:
            continue
        path = _monotone_path(n_ref, n_gen, rng)
        rec, moved, status = A.dtw_transfer(path, n_ref, n_gen, durations, m)
        K = sum(d > 0 for d in durations)
        assert status == (1 if n_ref < m * K else 0)
        seen.add(status)
        if status == 0:
            assert sum(rec) == n_ref and all((r >= m) if d > 0 else (r == 0) for r, d in zip(rec, durations))
            if m == 1 and moved == 0:                        # untouched starts: a symbol begins where the path first reaches it
                starts = np.concatenate([[0], np.cumsum(rec)])
                gen_starts = np.concatenate([[0], np.cumsum(durations)])
                for s, d in enumerate(durations):
                    if d > 0:
                        assert starts[s] == min(i for i, j in path if j == gen_starts[s])
    assert seen == {0, 1}


@pytest.mark.parametrize('case', A.active_span_cases(), ids=lambda c: c[0])
def test_active_span_oracle(case):
    name, energy, n, rel_db = case
    begin, end = A.active_span(energy, n, rel_db)
    want = {'all-zero': (0, 0), 'n=0': (0, 0), 'n=1': (0, 1), 'n=1-zero': (0, 0), 'negative-only': (0, 0), 'peak-first': (0, 2),
            'peak-last': (3, 5), 'at-threshold': (1, 5), 'rel-db-0': (1, 3), 'rel-db-6': (1, 3), 'burst-300': (70, 200),
            'burst-257': (70, 200), 'burst-64': None}[name]
    if want is not None:
        assert (begin, end) == want, (name, begin, end)
    assert 0 <= begin <= end <= n


# ---- the marker writer ------------------------------------------------------------------------------------------------------------------

SENTENCE = [['HH', 'AH0'], ',', ['W', 'ER1', 'L', 'D'], ' ', ['AH0'], '.', '~']
LAB = 'Hello, world a.\n'
#            HH AH0  ,  W ER1 L  D ' ' AH0 .  ~
DURATIONS = [3, 4, 5, 3, 6, 3, 4, 0, 7, 6, 2]


def _hp():
    return make_hparams()


def _rows(lines):
    return [line.rstrip('\n').split('\t') for line in lines]


def _symbols_read_back(lines, lab, hp):
    from daft_exprt.extract_features import marker_lines_span, update_markers
    sent_begin, _ = marker_lines_span(lines)
    out = update_markers('utt', lines, lab, sent_begin, [1] * len(lines), hp, logging.getLogger('test_align_host'))
    return None if out is None else [row[3] for row in out]


def _flat(sentence):
    return [s for item in sentence for s in (item if isinstance(item, list) else [item])]


def test_marker_rows():
    from daft_exprt.align import lab_words, markers_from_durations
    hp = _hp()
    words = lab_words(LAB)
    assert words == ['hello', 'world', 'a']
    n_samples = 70 * hp.hop_length
    lines = markers_from_durations(SENTENCE, words, DURATIONS, 5, n_samples, hp)
    assert all(ROW.match(line) for line in lines), lines
    rows = _rows(lines)
    # one row per phone, one <sil> row for the sounding comma, none for the silent whitespace, the full stop and the eos
    assert [r[2] for r in rows] == ['HH', 'AH0', 'SIL', 'W', 'ER1', 'L', 'D', 'AH0']
    assert [r[3] for r in rows] == ['hello', 'hello', '<sil>', 'world', 'world', 'world', 'world', 'a']
    assert [r[4] for r in rows] == ['0', '0', '1', '2', '2', '2', '2', '3']
    # a row ends where the next one begins, to the character; the times are the oracle's rule on the cumulated frames
    assert all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
    edges = np.concatenate([[0], np.cumsum(DURATIONS)]).tolist()
    want = [A.boundary_time(e, 5, n_samples, hp.hop_length, hp.sampling_rate) for e in edges]
    assert [r[0] for r in rows] == [want[0], want[1], want[2], want[3], want[4], want[5], want[6], want[8]]
    assert rows[-1][1] == want[9] and rows[2][1] == want[3]
    assert want[0] == '%.6f' % (4.5 * 256 / 22050)
    assert _symbols_read_back(lines, LAB, hp) == _flat(SENTENCE)


def test_leading_and_trailing_boundary_symbols_are_dropped_and_times_are_clipped():
    from daft_exprt.align import lab_words, markers_from_durations
    hp = _hp()
    sentence = [',', ['HH', 'AH0'], ['W'], '!', '~']            # (two adjacent words: nothing between them)
    lab = '"Hello w!"\n'
    durations = [4, 3, 3, 5, 6, 3]
    total = sum(durations)
    n_samples = (total - 1) * hp.hop_length + 17                 # the last boundary lies past the end of the recording
    lines = markers_from_durations(sentence, lab_words(lab), durations, 0, n_samples, hp)
    rows = _rows(lines)
    assert [r[2:] for r in rows] == [['HH', 'hello', '0'], ['AH0', 'hello', '0'], ['W', 'w', '1']]
    assert rows[0][0] == A.boundary_time(4, 0, n_samples) and rows[-1][1] == A.boundary_time(15, 0, n_samples)
    # the comma in front starts at frame 0: its begin would be clipped to 0; the eos behind ends at the last sample
    assert A.boundary_time(0, 0, n_samples) == '0.000000' and A.boundary_time(total, 0, n_samples) == '%.6f' % (n_samples / 22050)
    assert _symbols_read_back(lines, lab, hp) == ['HH', 'AH0', ' ', 'W', '!', '~']
    # sounding symbols between two words: one <sil> row over all of them
    sentence = [['HH'], ',', ' ', ['W']]
    lines = markers_from_durations(sentence, ['h', 'w'], [3, 2, 4, 3], 2, 10 ** 6, hp)
    rows = _rows(lines)
    assert [r[2:] for r in rows] == [['HH', 'h', '0'], ['SIL', '<sil>', '1'], ['W', 'w', '2']]
    assert rows[1][0] == A.boundary_time(3, 2, 10 ** 6) and rows[1][1] == A.boundary_time(9, 2, 10 ** 6)
    assert _symbols_read_back(lines, 'h, w', hp) == ['HH', ',', 'W', '~']


def test_what_cannot_be_written_returns_none():
    from daft_exprt.align import lab_words, markers_from_durations
    hp = _hp()
    assert markers_from_durations(SENTENCE, lab_words('Hello world.'), DURATIONS, 0, 10 ** 6, hp) is None      # two words for three groups
    assert markers_from_durations(SENTENCE, lab_words('Hello, big world a.'), DURATIONS, 0, 10 ** 6, hp) is None
    silent_phone = list(DURATIONS)
    silent_phone[4] = 0
    assert markers_from_durations(SENTENCE, lab_words(LAB), silent_phone, 0, 10 ** 6, hp) is None
    assert markers_from_durations(SENTENCE, lab_words(LAB), DURATIONS[:-1], 0, 10 ** 6, hp) is None
    assert markers_from_durations([',', '~'], [], [3, 3], 0, 10 ** 6, hp) is None


def test_the_reference_quantiser_gives_every_written_row_frames():
    ''' rows laid on the (frame - 1/2) hop grid, cropped and quantised the way `extract_features` does it: every row keeps a
        non-zero frame count and the counts add up to the frames of the crop '''
    from daft_exprt.align import markers_from_durations
    from daft_exprt.audio import crop_range
    from daft_exprt.symbols import arpabet_stressed
    hp = _hp()
    fs, hop = hp.sampling_rate, hp.hop_length
    rng = np.random.RandomState(5)
    pinned = 0
    for trial in range(400):
        K = int(rng.randint(4, 15))
        frames = rng.randint(3, 12, size=K).tolist()
        lead, tail, begin_frame = int(rng.randint(0, 6)), int(rng.randint(0, 6)), int(rng.randint(0, 40))
        sentence = [',', [arpabet_stressed[k] for k in range(K)], '~']
        n_samples = (begin_frame + lead + sum(frames) + tail) * hop - int(rng.randint(1, hop + 1))
        lines = markers_from_durations(sentence, ['word'], [lead] + frames + [tail], begin_frame, n_samples, hp)
        assert len(lines) == K
        rows = _rows(lines)
        sent_begin, sent_end = float(rows[0][0]), float(rows[-1][1])
        spans = [[float(r[0]) - sent_begin, float(r[1]) - sent_begin] for r in rows]
        n = crop_range(sent_begin, sent_end, fs, n_samples)[1]
        got = A.duration_to_integer(spans, n, fs, hp.filter_length, hop)
        assert len(got) == K and 0 not in got and sum(got) == 1 + n // hop, (trial, frames, begin_frame, got, n)
        total = 0
        for b, e in spans:
            total = total + (e - b)
        if int(total * fs) == n:                             # where the two sample counts agree: the rule as oracle/ states it
            assert got == REF.duration_to_integer(spans, fs, hp.filter_length, hop, True)
            pinned += 1
    assert pinned > 0


def test_align_cli_flags(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('align_cli', os.path.join(root, 'scripts', 'align.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    chk, text = tmp_path / 'ckpt', tmp_path / 'sentences.txt'
    chk.write_bytes(b'')
    text.write_text('u0|{HH AH0} ~\n', encoding='utf-8')
    args = cli.parse_args(['-chk', str(chk), '-dd', str(tmp_path), '-spks', 'A', 'B', '-tf', str(text)])
    assert (args.speakers, args.text_file, args.batch_size, args.min_frames, args.trim_db, args.overwrite) == \
        (['A', 'B'], [str(text)], 32, 3, -40.0, False)
    cli.check_args(args)
    args = cli.parse_args(['-chk', str(chk), '-dd', str(tmp_path), '-spks', 'A', '-tf', str(text), '-bs', '4', '-mf', '2', '-trim', '-30',
                           '--overwrite'])
    assert (args.batch_size, args.min_frames, args.trim_db, args.overwrite) == (4, 2, -30.0, True)
    for bad, word in ((['-tf', str(text), str(text), str(text)], 'one per speaker'), (['-tf', str(tmp_path / 'none.txt')], 'no such phonemised'),
                      (['-tf', str(text), '-mf', '0'], 'at least 1'), (['-tf', str(text), '-trim', '3'], 'at most 0')):
        with pytest.raises(SystemExit) as e:
            cli.check_args(cli.parse_args(['-chk', str(chk), '-dd', str(tmp_path), '-spks', 'A', 'B'] + bad))
        assert word in str(e.value), (bad, str(e.value))
