"""Phoneme alignments learned on the data set itself: a first checkpoint without an outside aligner.

Two small encoders -- one over the symbols, one over the natural-log mel -- give keys and queries; their soft alignment
(`soft_alignment`), the forward-sum loss over it (`forward_sum_loss`: the monotonic, blank-free CTC objective of RAD-TTS / "One
TTS Alignment to Rule Them All") and monotonic alignment search (`mas_path`, Glow-TTS) are the kernels of csrc/aligner.hip (K28).
`hard_durations` hands the MAS path to the existing `align.dtw_transfer_batch`, so the minimum-duration repair, `moved` and the
status codes are those of K27.  `Aligner.align_batch` returns what `align.align_batch` returns, so `align.align_data_set` writes
the `.markers` and the report with either; `train_aligner` trains one on a data-set directory and `scripts/train_aligner.py` is
the command line.

The encoders are plain torch modules (plumbing); the lattice work is HIP.  The arithmetic is pinned against
tests/aligner_oracle.py.  How close the boundaries come to a trained aligner's on real speech has NOT been measured: no accuracy
on speech is claimed.  No CPU fallback: without the HIP library / a GPU the device functions raise.
"""
import logging
import os
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt.align import dtw_transfer_batch
from daft_exprt.extract_features import mel_spectrogram_batch
from daft_exprt.generate import _symbol_ids, read_phonemised_sentences
from daft_exprt.recordings import empty_alignment, load_recordings, phonemised_by_speaker, sounding_crops, write_early_statuses

_logger = logging.getLogger(__name__)


def max_symbols():
    return int(H.lib().dx_aln_max_symbols())


def max_dim():
    return int(H.lib().dx_aln_max_dim())


def _lengths(n_frm, n_sym, B):
    assert n_frm.dtype == torch.int64 and n_sym.dtype == torch.int64 and n_frm.shape == (B,) and n_sym.shape == (B,)
    return n_frm.contiguous(), n_sym.contiguous()


def _check_logp(logp, n_frm, n_sym):
    H.require_gpu(logp, n_frm, n_sym)
    assert logp.dtype == torch.float32 and logp.dim() == 3
    return (logp.contiguous(),) + _lengths(n_frm, n_sym, logp.shape[0])


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------

def logprob_fwd(q, k, n_frm, n_sym, temperature, prior_sigma):
    ''' `dx_aln_logprob_fwd`: q (B, T, A), k (B, L, A) fp32 -> logp (B, T, L) fp32, dead cells 0 '''
    H.require_gpu(q, k, n_frm, n_sym)
    assert q.dtype == torch.float32 and k.dtype == torch.float32 and q.dim() == 3 and k.dim() == 3
    B, T, A = q.shape
    L = k.shape[1]
    assert k.shape == (B, L, A)
    n_frm, n_sym = _lengths(n_frm, n_sym, B)
    logp = torch.empty((B, T, L), dtype=torch.float32, device=q.device)
    H.check(H.lib().dx_aln_logprob_fwd(H.ptr(q.contiguous()), H.ptr(k.contiguous()), H.ptr(n_frm), H.ptr(n_sym), float(temperature),
                                       float(prior_sigma), H.ptr(logp), B, T, L, A, H.stream()))
    return logp


def logprob_bwd(q, k, logp, g, n_frm, n_sym, temperature):
    ''' `dx_aln_logprob_bwd`: g = dLoss/dlogp (B, T, L) -> (dq (B, T, A), dk (B, L, A)) '''
    H.require_gpu(q, k, logp, g, n_frm, n_sym)
    B, T, A = q.shape
    L = k.shape[1]
    assert logp.shape == (B, T, L) and g.shape == (B, T, L) and g.dtype == torch.float32 and logp.dtype == torch.float32
    n_frm, n_sym = _lengths(n_frm, n_sym, B)
    dq, dk = torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(k, memory_format=torch.contiguous_format)
    row_ws = torch.empty((B, T), dtype=torch.float32, device=q.device)
    H.check(H.lib().dx_aln_logprob_bwd(H.ptr(q.contiguous()), H.ptr(k.contiguous()), H.ptr(logp.contiguous()), H.ptr(g.contiguous()),
                                       H.ptr(n_frm), H.ptr(n_sym), float(temperature), H.ptr(dq), H.ptr(dk), H.ptr(row_ws), B, T, L, A,
                                       H.stream()))
    return dq, dk


def forward_sum(logp, n_frm, n_sym):
    ''' `dx_aln_forward_sum`: -> (alpha (B, T, L) fp32, loss (B,) fp32, status (B,) int32) '''
    logp, n_frm, n_sym = _check_logp(logp, n_frm, n_sym)
    B, T, L = logp.shape
    alpha = torch.empty_like(logp)
    loss = torch.empty((B,), dtype=torch.float32, device=logp.device)
    status = torch.empty((B,), dtype=torch.int32, device=logp.device)
    H.check(H.lib().dx_aln_forward_sum(H.ptr(logp), H.ptr(n_frm), H.ptr(n_sym), H.ptr(alpha), H.ptr(loss), H.ptr(status), B, T, L,
                                       H.stream()))
    return alpha, loss, status


def forward_sum_bwd(logp, alpha, w, n_frm, n_sym):
    ''' `dx_aln_forward_sum_bwd`: w (B,) fp32 = dLoss/dloss[b] -> dlogp (B, T, L) '''
    logp, n_frm, n_sym = _check_logp(logp, n_frm, n_sym)
    B, T, L = logp.shape
    assert alpha.shape == (B, T, L) and alpha.dtype == torch.float32 and alpha.is_contiguous() and w.shape == (B,) and w.dtype == torch.float32
    dlogp = torch.empty_like(logp)
    H.check(H.lib().dx_aln_forward_sum_bwd(H.ptr(logp), H.ptr(alpha), H.ptr(w.contiguous()), H.ptr(n_frm), H.ptr(n_sym), H.ptr(dlogp), B, T,
                                           L, H.stream()))
    return dlogp


def mas_path(logp, n_frm, n_sym):
    ''' `dx_aln_mas`: -> (path (B, T + L - 1, 2) int32 and path_len (B,) int32 in the layout of `evaluate.dtw_align_batch`: the cells
        (frame, symbol), one per frame; score (B,) fp32; status (B,) int32: 0 ok, 1 fewer frames than symbols, 2 an empty axis) '''
    logp, n_frm, n_sym = _check_logp(logp, n_frm, n_sym)
    B, T, L = logp.shape
    dev = logp.device
    path = torch.empty((B, T + L - 1, 2), dtype=torch.int32, device=dev)
    path_len = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    words = T * ((L + 63) // 64)
    ws = torch.empty((B, words), dtype=torch.int64, device=dev)
    H.check(H.lib().dx_aln_mas(H.ptr(logp), H.ptr(n_frm), H.ptr(n_sym), H.ptr(score), H.ptr(path), H.ptr(path_len), H.ptr(status),
                               H.ptr(ws), 8 * words, B, T, L, H.stream()))
    return path, path_len, score, status


class _SoftAlignment(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, n_frm, n_sym, temperature, prior_sigma):
        logp = logprob_fwd(q, k, n_frm, n_sym, temperature, prior_sigma)
        ctx.save_for_backward(q, k, logp, n_frm, n_sym)
        ctx.temperature = float(temperature)
        return logp

    @staticmethod
    def backward(ctx, g):
        q, k, logp, n_frm, n_sym = ctx.saved_tensors
        dq, dk = logprob_bwd(q, k, logp, g.float().contiguous(), n_frm, n_sym, ctx.temperature)
        return dq, dk, None, None, None, None


class _ForwardSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, n_frm, n_sym):
        alpha, loss, status = forward_sum(logp, n_frm, n_sym)
        ctx.save_for_backward(logp, alpha, n_frm, n_sym)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    def backward(ctx, w, _):
        logp, alpha, n_frm, n_sym = ctx.saved_tensors
        return forward_sum_bwd(logp, alpha, w.float().contiguous(), n_frm, n_sym), None, None


def soft_alignment(q, k, n_frm, n_sym, temperature, prior_sigma):
    ''' log-probabilities of the symbols per frame, differentiable in q (B, T, A) and k (B, L, A): logp (B, T, L),
        log_softmax over l < n_sym of -temperature |q_t - k_l|^2 + prior(t, l) (K28); 0 in the dead cells '''
    return _SoftAlignment.apply(q, k, n_frm, n_sym, float(temperature), float(prior_sigma))


def forward_sum_loss(logp, n_frm, n_sym):
    ''' the forward-sum objective, differentiable in logp: returns (mean over the rows with status 0 of loss[b] / n_frm[b],
        the number of rows with another status -- fewer frames than symbols, or an empty axis -- which contribute nothing) '''
    loss, status = _ForwardSum.apply(logp, n_frm, n_sym)
    ok = status == 0
    per_frame = torch.where(ok, loss / n_frm.clamp(min=1).to(loss.dtype), torch.zeros_like(loss))
    return per_frame.sum() / ok.sum().clamp(min=1).to(loss.dtype), (~ok).sum()


def hard_durations(logp, n_frm, n_sym, min_frames=1):
    ''' MAS, then `align.dtw_transfer_batch` with every symbol sounding and one "synthesis" frame long (gen_durations all 1,
        n_gen = n_sym).  Returns (durations (B, L) int64: the frames of every symbol, at least min_frames each where status is 0;
        moved, status: as `dtw_transfer_batch`; score (B,) fp32 and mas_status (B,) int32 of `mas_path`) '''
    path, path_len, score, mas_status = mas_path(logp, n_frm, n_sym)
    ones = torch.ones((logp.shape[0], logp.shape[2]), dtype=torch.int64, device=logp.device)
    durations, moved, status = dtw_transfer_batch(path, path_len, n_frm.contiguous(), n_sym.contiguous(), ones, n_sym.contiguous(),
                                                  min_frames)
    return durations, moved, status, score, mas_status


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

def _conv(x, conv):
    ''' a Conv1d (kernel 1 or 3, same padding) over time-major x (B, N, C) as one matrix product over the stacked taps '''
    w = conv.weight
    if w.shape[2] == 1:
        return F.linear(x, w[:, :, 0], conv.bias)
    pad = F.pad(x, (0, 0, 1, 1))
    taps = torch.cat([pad[:, :-2], pad[:, 1:-1], pad[:, 2:]], dim=2)
    return F.linear(taps, w.permute(0, 2, 1).reshape(w.shape[0], -1), conv.bias)


class Aligner(nn.Module):
    ''' key encoder: embedding -> Conv1d(3) -> ReLU -> Conv1d(1);  query encoder over the natural-log mel: Conv1d(3) -> ReLU ->
        Conv1d(3) -> ReLU -> Conv1d(1); both masked at the sequence ends in front of every convolution '''
    def __init__(self, n_symbols, n_mel, hidden=256, att_dim=80, temperature=0.05, prior_sigma=0.2):
        super().__init__()
        self.args = dict(n_symbols=int(n_symbols), n_mel=int(n_mel), hidden=int(hidden), att_dim=int(att_dim),
                         temperature=float(temperature), prior_sigma=float(prior_sigma))
        self.temperature, self.prior_sigma = float(temperature), float(prior_sigma)
        self.embedding = nn.Embedding(n_symbols, hidden)
        self.key_1, self.key_2 = nn.Conv1d(hidden, hidden, 3, padding=1), nn.Conv1d(hidden, att_dim, 1)
        self.query_1, self.query_2 = nn.Conv1d(n_mel, hidden, 3, padding=1), nn.Conv1d(hidden, hidden, 3, padding=1)
        self.query_3 = nn.Conv1d(hidden, att_dim, 1)

    def encode(self, symbols, n_sym, mel, n_frm):
        ''' symbols (B, L) int64, mel (B, n_mel, T) natural-log -> (q (B, T, A), k (B, L, A)) fp32 contiguous '''
        ml = (torch.arange(symbols.shape[1], device=symbols.device)[None] < n_sym[:, None]).to(torch.float32)[:, :, None]
        mt = (torch.arange(mel.shape[2], device=mel.device)[None] < n_frm[:, None]).to(torch.float32)[:, :, None]
        k = _conv(torch.relu(_conv(self.embedding(symbols) * ml, self.key_1)) * ml, self.key_2)
        x = mel.float().transpose(1, 2) * mt
        q = _conv(torch.relu(_conv(torch.relu(_conv(x, self.query_1)) * mt, self.query_2)) * mt, self.query_3)
        return q.contiguous(), k.contiguous()

    def forward(self, symbols, n_sym, mel, n_frm, prior_sigma=None):
        ''' logp (B, T, L) of `soft_alignment`; prior_sigma: the constructor's, or 0 for no prior '''
        q, k = self.encode(symbols, n_sym, mel, n_frm)
        return soft_alignment(q, k, n_frm, n_sym, self.temperature, self.prior_sigma if prior_sigma is None else prior_sigma)

    def align_batch(self, symbols, input_lengths, wavs, n_samples, speaker_ids, hparams, min_frames=3, trim_db=-40.0):
        ''' the dict of `align.ALIGN_KEYS` with the meanings of `align.align_batch`: the same front end (frame energies, sounding
            stretch [begin, end), the crop's mel) and early statuses 3 / 4; gen_durations is 1 per symbol and frames_gen the symbol
            count, path_cost = -score / frames of the MAS path (prior off), status 1 also where the crop has fewer frames than the
            utterance symbols.  speaker_ids is accepted and ignored. '''
        H.require_gpu(symbols, input_lengths, wavs)
        dev = wavs.device
        B, L = symbols.shape
        out = empty_alignment(B, L, dev)
        with torch.no_grad():                                     # (no dropout or norm layer: nothing depends on the training mode)
            status, rows, begin, mel, n_rec = sounding_mels(wavs, n_samples, hparams, trim_db)
            if rows:
                idx = torch.tensor(rows, dtype=torch.int64, device=dev)
                n_sym = input_lengths[idx].contiguous()
                logp = self(symbols[idx].contiguous(), n_sym, mel, n_rec, prior_sigma=0.)
                durations, moved, st, score, mas_status = hard_durations(logp, n_rec, n_sym, min_frames)
                st = torch.where(mas_status == 1, torch.ones_like(st), st)
                ok = st == 0
                out['rec_durations'][idx] = torch.where(ok[:, None], durations, torch.zeros_like(durations))
                out['moved'][idx], out['status'][idx] = torch.where(ok, moved, torch.zeros_like(moved)), st
                out['gen_durations'][idx] = (torch.arange(L, device=dev)[None] < n_sym[:, None]).to(torch.int64)
                out['path_cost'][idx] = -score / n_rec.clamp(min=1).float()
                out['begin'][idx] = torch.tensor(begin, dtype=torch.int64, device=dev)
                out['frames'][idx], out['frames_gen'][idx] = n_rec, n_sym
        write_early_statuses(out, status)
        return out


def sounding_mels(wavs, n_samples, hparams, trim_db=-40.0):
    ''' the front end of `align.align_batch` (`recordings.sounding_crops`: its arguments, status, rows and begin) and the crops'
        natural-log mel (len(rows), n_mel, T) fp32 with n_rec (len(rows),) int64, their frames '''
    status, rows, begin, cropped, lengths, crop = sounding_crops(wavs, n_samples, hparams, trim_db)
    if not rows:
        return status, [], [], None, None
    mel, _, n_rec = mel_spectrogram_batch(cropped, crop[:, 1].contiguous(), hparams, min_samples=min(lengths))
    return status, rows, begin, mel, n_rec


# ---- training and checkpoints ----------------------------------------------------------------------------------------------------------

def save_aligner(aligner, path):
    ''' the weights and the constructor arguments '''
    torch.save({'args': dict(aligner.args), 'state_dict': {k: v.detach().cpu() for k, v in aligner.state_dict().items()}}, path)


def load_aligner(path, device='cuda:0'):
    chk = torch.load(path, map_location='cpu')
    aligner = Aligner(**chk['args'])
    aligner.load_state_dict(chk['state_dict'])
    return aligner.to(H.device(device))


def _collate(items, device):
    ''' items: [(ids (L_b,) int64, mel (n_mel, T_b) fp32)] on the device -> symbols (B, L), n_sym, mel (B, n_mel, T), n_frm '''
    B, L, T = len(items), max(len(i[0]) for i in items), max(i[1].shape[1] for i in items)
    symbols = torch.zeros((B, L), dtype=torch.int64, device=device)
    mel = torch.zeros((B, items[0][1].shape[0], T), dtype=torch.float32, device=device)
    for b, (ids, m) in enumerate(items):
        symbols[b, :len(ids)], mel[b, :, :m.shape[1]] = ids, m
    n_sym = torch.tensor([len(i[0]) for i in items], dtype=torch.int64, device=device)
    n_frm = torch.tensor([i[1].shape[1] for i in items], dtype=torch.int64, device=device)
    return symbols, n_sym, mel, n_frm


def train_step(aligner, optimizer, items, device):
    ''' one Adam step on a list of (ids, mel) items; returns (the loss, the rows that contributed nothing) as device tensors '''
    symbols, n_sym, mel, n_frm = _collate(items, device)
    loss, skipped = forward_sum_loss(aligner(symbols, n_sym, mel, n_frm), n_frm, n_sym)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss.detach(), skipped


def train_aligner(dataset_dir, speakers, phonemised_files, hparams, steps=2000, batch_size=32, lr=1e-3, temperature=0.05,
                  prior_sigma=0.2, seed=1234, hidden=256, att_dim=80, trim_db=-40.0, log_every=100, device='cuda:0'):
    ''' trains an `Aligner` on the recordings `align.align_data_set` reads -- `<dataset_dir>/<speaker>/wavs/NAME.wav` for the
        `NAME|...` lines of the speaker's phonemised file (phonemised_files as there) -- and returns it.  The mels of the sounding
        stretches are extracted once, batch_size recordings at a time through `recordings.load_recordings` and `sounding_mels`, and
        stay on the device; every step draws batch_size of them (a seeded permutation per step), Adam at `lr`, the loss logged every
        `log_every` steps.  Recordings without a wav, with status 3 / 4 or with fewer frames than symbols are left out. '''
    dev = H.device(device)
    fs = int(hparams.sampling_rate)
    speakers = list(speakers)
    phonemised_files = phonemised_by_speaker(phonemised_files, speakers)
    items, left_out = [], 0
    for speaker in speakers:
        wavs_dir = os.path.join(dataset_dir, speaker, 'wavs')
        if not os.path.isdir(wavs_dir):
            raise FileNotFoundError(f'There is no such directory: {wavs_dir}')
        sentences, names = read_phonemised_sentences(phonemised_files[speaker], hparams.symbols)
        todo = [SimpleNamespace(wav_file=os.path.join(wavs_dir, f'{name}.wav'), ids=_symbol_ids(sentence, hparams))
                for sentence, name in zip(sentences, names)]
        left_out += sum(not os.path.isfile(u.wav_file) for u in todo)
        todo = [u for u in todo if os.path.isfile(u.wav_file)]
        for pos in range(0, len(todo), int(batch_size)):
            utts = todo[pos: pos + int(batch_size)]
            symbols, _, wavs, n_total = load_recordings(utts, fs, dev)
            with torch.no_grad():
                status, rows, _, mel, n_rec = sounding_mels(wavs, n_total, hparams, trim_db)
            frames = n_rec.tolist() if rows else []
            for i, b in enumerate(rows):
                if len(utts[b].ids) <= frames[i] and 0 < len(utts[b].ids) <= max_symbols():
                    items.append((symbols[b, :len(utts[b].ids)].clone(), mel[i, :, :frames[i]].clone()))
        left_out += len(todo)
    left_out -= len(items)
    if not items:
        raise ValueError('train_aligner: no recording to train on')
    _logger.info(f'train_aligner: {len(items)} recordings on the device, {left_out} left out')
    torch.manual_seed(int(seed))
    aligner = Aligner(len(hparams.symbols), int(hparams.n_mel_channels), hidden, att_dim, temperature, prior_sigma).to(dev)
    aligner.train()
    optimizer = torch.optim.Adam(aligner.parameters(), lr=float(lr))
    g = torch.Generator().manual_seed(int(seed))
    for step in range(int(steps)):
        idx = torch.randperm(len(items), generator=g)[:int(batch_size)].tolist()
        loss, skipped = train_step(aligner, optimizer, [items[i] for i in idx], dev)
        if log_every and (step % int(log_every) == 0 or step == int(steps) - 1):
            _logger.info(f'train_aligner: step {step} -- forward-sum loss per frame {float(loss):.5f} -- rows without a path {int(skipped)}')
    return aligner
