"""What a validation pass shows beyond its loss: the content of `DaftExprtLogger.log_validation` (`logger.py:34-157`) as data.

The reference keeps every validation batch's outputs on the GPU -- the dense (B, L, T) alignments of the whole set included --
and reduces them in numpy for TensorBoard figures.  Here each batch is reduced on the device while it is there
(`csrc/validation.hip`) and only small results are kept:

  * the FiLM gammas / betas of every utterance (rows x nb_blocks x width floats per module), concatenated on the device and
    turned into 50-bin histograms per module, block and gamma | beta at the end (`film_histograms`);
  * three numbers per utterance that say how closely the Gaussian upsampler's alignment follows the integer durations it was
    teacher-forced with (`alignment_scores`);
  * one utterance of one batch, chosen BEFORE the loop, as the reference's scatter / image figures show it.

`ValidationReport.write` leaves `iter_<iteration>.npz` and returns scalars for `metrics.jsonl`; `figures` draws PNGs when
matplotlib can be imported and is never needed for anything else.
"""
import contextlib
import logging
import os
import random
import time

import numpy as np
import torch

from daft_exprt import _hip as H
from daft_exprt import ops

_logger = logging.getLogger(__name__)
MODULES = ('encoder', 'prosody_predictor', 'decoder')     # outputs[1][1..3], logger.py:100-116
BINS = ops.FILM_BINS


def histogram_edges(minmax):
    ''' (G, 2) min / max -> (G, 51) float64 edges, as numpy.histogram builds them for bins=50: linspace in double between the
        extremes, between lo - 0.5 and hi + 0.5 when they coincide '''
    minmax = np.asarray(minmax, dtype=np.float64)
    edges = np.empty((minmax.shape[0], BINS + 1), dtype=np.float64)
    for g, (lo, hi) in enumerate(minmax):
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        edges[g] = np.linspace(lo, hi, BINS + 1)
    return edges


def histogram_density(counts, edges):
    ''' counts / (n x bin width): what `hist(..., density=True)` draws (`utils.py:28`); zeros for an empty histogram '''
    counts = np.asarray(counts)
    n = counts.sum(axis=-1, keepdims=True).astype(np.float64)
    return np.where(n > 0, counts / (np.maximum(n, 1.) * np.diff(edges, axis=-1)), 0.)


def film_histograms(films):
    ''' films (rows, nb_blocks, width) device tensor, a block's first width / 2 values its gammas and the rest its betas
        (`logger.py:118-125`).  Returns numpy arrays indexed [block, 0 gammas | 1 betas]: counts (.., 50) int64, edges (.., 51)
        float64, density (.., 50) float64, finite (nb_blocks, 2) bool, minmax (.., 2) float32.  A group that holds a NaN or an
        infinity has finite False and zero counts (numpy.histogram raises there; the caller logs it and training goes on). '''
    H.require_gpu(films)
    films = films.detach().float().contiguous()
    nb = films.shape[1]
    minmax_dev, finite_dev = ops.film_hist_range(films)
    minmax, finite = minmax_dev.cpu().numpy(), finite_dev.cpu().numpy()       # 2 G values: the only round trip between the two passes
    edges = histogram_edges(minmax)
    counts = ops.film_hist_count(films, torch.from_numpy(edges).to(films.device), finite_dev).cpu().numpy()
    return {'counts': counts.reshape(nb, 2, BINS), 'edges': edges.reshape(nb, 2, BINS + 1),
            'density': histogram_density(counts, edges).reshape(nb, 2, BINS), 'finite': finite.reshape(nb, 2).astype(bool),
            'minmax': minmax.reshape(nb, 2, 2)}


def alignment_scores(weights, durations_int, in_lengths, out_lengths):
    ''' per utterance (frames, hits, mass) device tensors, see `dx_alignment_score`: the frames the integer durations hand out,
        those among them whose strongest symbol is their owner, and the mean weight the owners get '''
    H.require_gpu(weights, durations_int, in_lengths, out_lengths)
    return ops.alignment_score(weights.detach().float().contiguous(), durations_int.long().contiguous(),
                               in_lengths.long().contiguous(), out_lengths.long().contiguous())


def target_alignment(durations_int, nb_frames):
    ''' (L, nb_frames) 0 / 1 matrix: symbol l owns the next durations_int[l] frames (`logger.py:92-98`) '''
    durations_int = np.asarray(durations_int).astype(np.int64)
    target = np.zeros((len(durations_int), int(nb_frames)), dtype=np.float32)
    col = 0
    for l, d in enumerate(durations_int):
        target[l, col: col + max(int(d), 0)] = 1.
        col += max(int(d), 0)
    return target


class ValidationReport(object):
    ''' accumulates one validation pass (`add_batch` per batch, from `train.validate`), then `write` and `figures`.

        The batch and the utterance the per-utterance figures show are drawn here, before the loop, from
        `random.Random(hparams.seed + iteration)`: only that batch's slices are copied off the device and no batch's dense
        alignment outlives its iteration (the reference draws them afterwards, from the outputs of every batch it kept). '''
    def __init__(self, hparams, iteration, nb_batches):
        rng = random.Random(int(getattr(hparams, 'seed', 0)) + int(iteration))
        self.iteration = int(iteration)
        self.pick_batch = rng.randrange(max(1, int(nb_batches)))
        self._pick_frac = rng.random()                      # position inside the picked batch, whose size is only known there
        self._films = {m: [] for m in MODULES}              # per batch (B, nb_blocks, width) device tensors
        self._scores = []                                   # per batch (frames, hits, mass) device tensors
        self._seen = 0
        self.seconds, self._timing = 0., False              # host time spent in this report's calls (`train` logs it)
        self.films = self.film_stats = self.frames = self.hits = self.mass = None    # numpy, filled by `finish`
        self.sample = None

    @classmethod
    def from_results(cls, hparams, iteration, films, film_stats, frames, hits, mass, sample=None):
        ''' a report over results that already are numpy (what `finish` leaves): films {module: `film_histograms` dict},
            film_stats {module: {'mean', 'std'} (nb_blocks, 2)}, per-utterance frames / hits / mass, sample dict or None '''
        self = cls(hparams, iteration, 1)
        self.films, self.film_stats, self.sample = films, film_stats, sample
        self.frames, self.hits, self.mass = np.asarray(frames, np.int64), np.asarray(hits, np.int64), np.asarray(mass, np.float32)
        self._films = self._scores = None
        return self

    @contextlib.contextmanager
    def _timed(self):
        if self._timing:            # (a timed call inside a timed call: the outer one counts)
            yield
            return
        self._timing, begin = True, time.time()
        try:
            yield
        finally:
            self.seconds += time.time() - begin
            self._timing = False

    def add_batch(self, inputs, targets, outputs):
        ''' inputs / targets as `DaftExprt.parse_batch` returns them, outputs = model(inputs) '''
        with self._timed():
            self._add_batch(inputs, targets, outputs)

    def _add_batch(self, inputs, targets, outputs):
        _, films, (dur_p, energy_p, pitch_p, in_lengths), (mel_p, out_lengths), weights = outputs
        for m, film in zip(MODULES, films[1:4]):
            self._films[m].append(film.detach().float().clone())
        self._scores.append(alignment_scores(weights, inputs[2], in_lengths, out_lengths))
        if self._seen == self.pick_batch:
            B = mel_p.shape[0]
            u = min(int(self._pick_frac * B), B - 1)
            L, T = int(in_lengths[u]), int(out_lengths[u])
            host = lambda t: t.detach().float().cpu().numpy()
            dur_t, energy_t, pitch_t, mel_t = targets[0], targets[1], targets[2], targets[3]
            dint = inputs[2][u, :L].cpu().numpy()
            self.sample = {'sample_batch': np.int64(self._seen), 'sample_index': np.int64(u),
                           'duration_target': host(dur_t[u, :L]), 'duration_pred': host(dur_p[u, :L]),
                           'energy_target': host(energy_t[u, :L]), 'energy_pred': host(energy_p[u, :L]),
                           'pitch_target': host(pitch_t[u, :L]), 'pitch_pred': host(pitch_p[u, :L]),
                           'mel_target': host(mel_t[u, :, :T]), 'mel_pred': host(mel_p[u, :, :T]),
                           'alignment_pred': host(weights[u, :L, :T]), 'alignment_target': target_alignment(dint, T),
                           'sample_durations_int': dint}
        self._seen += 1

    def finish(self):
        ''' the device reductions over what `add_batch` collected; the results are numpy from here on '''
        if self.films is not None:
            return
        with self._timed():
            self._finish()

    def _finish(self):
        self.films, self.film_stats = {}, {}
        for m in MODULES:
            film = torch.cat(self._films[m], dim=0)
            rows, nb, width = film.shape
            self.films[m] = film_histograms(film)
            halves = film.double().view(rows, nb, 2, width // 2)
            var, mean = torch.var_mean(halves, dim=(0, 3), unbiased=False)
            self.film_stats[m] = {'mean': mean.cpu().numpy(), 'std': var.sqrt().cpu().numpy()}
            for blk, half in zip(*np.nonzero(~self.films[m]['finite'])):
                _logger.warning(f'Validation report {self.iteration}: non-finite FiLM {("gammas", "betas")[half]} in {m} block {blk} '
                                f'-- no histogram for this group')
        frames, hits, mass = (torch.cat(parts).cpu().numpy() for parts in zip(*self._scores))
        self.frames, self.hits, self.mass = frames, hits, mass
        self._films, self._scores = None, None

    def arrays(self):
        ''' everything `write` stores, as {key: numpy array} '''
        self.finish()
        out = {'iteration': np.int64(self.iteration), 'alignment_frames': self.frames, 'alignment_hits': self.hits,
               'alignment_mass': self.mass}
        for m in MODULES:
            for key in ('counts', 'edges', 'density', 'finite'):
                out[f'film_{m}_{key}'] = self.films[m][key]
            out[f'film_{m}_mean'], out[f'film_{m}_std'] = self.film_stats[m]['mean'], self.film_stats[m]['std']
        out.update(self.sample or {})
        return out

    def scalars(self):
        self.finish()
        live = self.frames > 0
        out = {'DaftExprt.validation/alignment_mass': float(self.mass[live].astype(np.float64).mean()) if live.any() else 0.,
               'DaftExprt.validation/alignment_hit_rate': float(self.hits.sum()) / float(self.frames.sum()) if live.any() else 0.}
        for m in MODULES:
            for blk in range(self.film_stats[m]['mean'].shape[0]):
                for half, name in enumerate(('gamma', 'beta')):
                    for stat in ('mean', 'std'):
                        out[f'DaftExprt.film/{m}/block{blk}/{name}_{stat}'] = float(self.film_stats[m][stat][blk, half])
        return out

    def path(self, directory):
        return os.path.join(directory, f'iter_{self.iteration:07d}.npz')

    def write(self, directory, iteration=None):
        ''' `<directory>/iter_<iteration>.npz` (keys: `arrays`); returns the scalars of this validation '''
        if iteration is not None:
            self.iteration = int(iteration)
        with self._timed():
            os.makedirs(directory, exist_ok=True)
            np.savez(self.path(directory), **self.arrays())
            return self.scalars()

    def figures(self, directory, iteration=None):
        ''' the figures of `logger.py:114-157` as `<directory>/iter_<iteration>_<tag>.png`: gammas and betas per module, durations,
            energies, pitch, mel-spectrogram, alignments.  Returns the list of files, or None when matplotlib is not installed. '''
        if iteration is not None:
            self.iteration = int(iteration)
        try:
            import matplotlib  # noqa: F401
            from matplotlib.backends.backend_agg import FigureCanvasAgg     # the Agg canvas, whatever backend the process has selected
            from matplotlib.figure import Figure
        except ImportError:
            _logger.info('matplotlib is not installed: the validation report is written as data only')
            return None
        with self._timed():
            return self._figures(directory, Figure, FigureCanvasAgg)

    def _figures(self, directory, Figure, FigureCanvasAgg):
        self.finish()
        os.makedirs(directory, exist_ok=True)
        files = []

        def save(fig, tag):
            FigureCanvasAgg(fig)
            files.append(os.path.join(directory, f'iter_{self.iteration:07d}_{tag}.png'))
            fig.savefig(files[-1])

        for m in MODULES:
            hist = self.films[m]
            nb = hist['counts'].shape[0]
            for half, name in enumerate(('gammas', 'betas')):
                fig = Figure(figsize=(16, 4))
                for blk, ax in enumerate(fig.subplots(1, nb, squeeze=False)[0]):
                    e = hist['edges'][blk, half]
                    ax.bar(e[:-1], hist['density'][blk, half], width=np.diff(e), align='edge')
                    ax.set(xlabel=f'Value -- Block {blk}', ylabel='Frequency')
                save(fig, f'{m}_film_{name}')
        s = self.sample
        if s is not None:
            for tag, key, label in (('durations', 'duration', 'Duration (sec)'), ('energies', 'energy', 'Energy (normalized)'),
                                    ('pitch', 'pitch', 'Pitch (normalized)')):
                fig = Figure(figsize=(16, 4))
                ax = fig.subplots()
                for values, color, who in ((s[f'{key}_target'], 'blue', 'ground-truth'), (s[f'{key}_pred'], 'red', 'predicted')):
                    ax.scatter(np.arange(len(values)), values, color=color, marker='o', label=who)
                ax.legend()
                ax.set(xlabel='Symbol ID', ylabel=label)
                save(fig, tag)
            for tag, pair, xl, yl in (('mel-spectrogram', ('mel_target', 'mel_pred'), ('Frames -- Ground Truth', 'Frames -- Predicted'), 'Frequencies'),
                                      ('alignments', ('alignment_target', 'alignment_pred'),
                                       ('Frames -- Ground Truth', 'Frames -- Predicted (from Ground Truth)'), 'Symbol ID')):
                fig = Figure(figsize=(16, 4))
                for ax, key, x in zip(fig.subplots(1, 2), pair, xl):
                    ax.imshow(s[key], aspect='auto', origin='lower', interpolation='none')
                    ax.set(xlabel=x, ylabel=yl)
                save(fig, tag)
        return files
