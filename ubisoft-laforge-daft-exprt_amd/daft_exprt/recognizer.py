"""Intelligibility: a CTC phone recogniser trained on the corpus's own feature files, and the phone error rate of a synthesis
against the phones it was asked for, on the GPU.  The reference has no counterpart.

MCD and the prosody scores say how close a synthesis is to a recording; nothing said whether its phones can be heard.  Here a small
convolutional recogniser over the natural-log mel is trained with the CTC loss on the (mel, symbols) pairs the data loader reads,
decoded greedily, and the decode is compared with the input phones by edit distance: substitutions, deletions, insertions, and
their sum over the reference length, the phone error rate (PER).  It needs no recording of the sentence that is scored.  The
lattice work -- the CTC loss with its gradient at utterance length (`uctc_loss`), the greedy decode (`uctc_greedy`) and the edit
distance (`edit_distance`) -- are the kernels of csrc/recognizer.hip (K31); the encoder is plain torch (plumbing, as in
`aligner.Aligner`).  `train_recognizer` trains one from file lists, `phone_error_rates` scores a batch, and
`scripts/train_recognizer.py`, `scripts/evaluate.py -rec` and `scripts/synthesize.py -rec` are the command lines.

The arithmetic is pinned against tests/ctc_oracle.py and tests/recognizer_oracle.py.  What nobody has measured: the recogniser's
PER on real speech, and how its PER on a synthesis tracks what listeners understand -- neither is claimed.  A recogniser trained on
a small corpus errs on recordings too: read a synthesis's PER beside the PER of the recording (`evaluate.copy_synthesis_scores`
reports both).  No CPU fallback: without the HIP library / a GPU the device functions raise.
"""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt.g2p import _conv, phones_of

_logger = logging.getLogger(__name__)

PER_KEYS = ('sub', 'del', 'ins', 'n_ref', 'per', 'n_hyp')


def limits():
    ''' (steps, labels, classes): the largest T, U and V (blank included) the K31 CTC kernels admit '''
    lib = H.lib()
    return int(lib.dx_uctc_max_steps()), int(lib.dx_uctc_max_labels()), int(lib.dx_uctc_max_classes())


def edit_max_len():
    ''' the longest sequence `edit_distance` takes on either side '''
    return int(H.lib().dx_edit_max_len())


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------

def _check_logits(who, logits, n_steps, U=0):
    H.require_gpu(logits, n_steps)
    assert logits.dtype == torch.float32 and logits.dim() == 3 and n_steps.dtype == torch.int64 and n_steps.shape == (logits.shape[0],)
    B, T, V = logits.shape
    max_t, max_u, max_v = limits()
    if T > max_t or U > max_u or V > max_v:
        raise ValueError(f'{who}: {T} steps (at most {max_t}), {U} labels (at most {max_u}) or {V} classes (at most {max_v})')
    return logits.contiguous(), n_steps.contiguous()


def uctc_loss_and_grad(logits, n_steps, labels, n_labels, w=None):
    ''' `dx_uctc_loss`: logits (B, T, V) fp32, labels (B, U) int64 in [1, V - 1], w (B,) fp32 (default: ones) ->
        (loss (B,) fp32, status (B,) int32, grad (B, T, V) fp32 = w[b] dloss[b] / dlogits); blank is class 0 '''
    H.require_gpu(labels, n_labels)
    B, T, V = logits.shape
    assert labels.dtype == torch.int64 and labels.dim() == 2 and labels.shape[0] == B and n_labels.dtype == torch.int64 and n_labels.shape == (B,)
    U = labels.shape[1]
    logits, n_steps = _check_logits('uctc_loss', logits, n_steps, U)
    dev = logits.device
    w = torch.ones((B,), dtype=torch.float32, device=dev) if w is None else w.float().contiguous()
    assert w.shape == (B,)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    grad = torch.empty_like(logits)
    ws = torch.empty((2, B, T, 2 * U + 1), dtype=torch.float32, device=dev)
    H.check(H.lib().dx_uctc_loss(H.ptr(logits), H.ptr(n_steps), H.ptr(labels.contiguous()) if U else None, H.ptr(n_labels.contiguous()),
                                 H.ptr(w), H.ptr(loss), H.ptr(status), H.ptr(grad), H.ptr(ws), B, T, U, V, H.stream()))
    return loss, status, grad


def uctc_greedy(logits, n_steps):
    ''' `dx_uctc_greedy`: -> (ids (B, T) int32: the arg-max path with repeats collapsed and blanks dropped, zeros behind n_out;
        n_out (B,) int32; score (B,) fp32: the summed log-probability of the arg-max path) '''
    logits, n_steps = _check_logits('uctc_greedy', logits, n_steps)
    B, T, V = logits.shape
    ids = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    n_out = torch.empty((B,), dtype=torch.int32, device=logits.device)
    score = torch.empty((B,), dtype=torch.float32, device=logits.device)
    H.check(H.lib().dx_uctc_greedy(H.ptr(logits), H.ptr(n_steps), H.ptr(ids), H.ptr(n_out), H.ptr(score), B, T, V, H.stream()))
    return ids, n_out, score


def edit_distance(ref, n_ref, hyp, n_hyp):
    ''' `dx_edit_distance`: ref (B, R) / hyp (B, H) int32 device tensors with n_ref / n_hyp (B,) int64 -> counts (B, 4) int32:
        substitutions, deletions, insertions and matches of the cheapest alignment of ref[b, :n_ref[b]] with hyp[b, :n_hyp[b]]
        (among equal costs the diagonal, then the deletion, then the insertion) '''
    H.require_gpu(ref, n_ref, hyp, n_hyp)
    assert ref.dtype == torch.int32 and hyp.dtype == torch.int32 and ref.dim() == 2 and hyp.dim() == 2 and ref.shape[0] == hyp.shape[0]
    B, R = ref.shape
    Hn = hyp.shape[1]
    assert n_ref.dtype == torch.int64 and n_hyp.dtype == torch.int64 and n_ref.shape == (B,) and n_hyp.shape == (B,)
    if max(R, Hn) > edit_max_len():
        raise ValueError(f'edit_distance: sequences of {R} and {Hn} entries (at most {edit_max_len()})')
    counts = torch.empty((B, 4), dtype=torch.int32, device=ref.device)
    H.check(H.lib().dx_edit_distance(H.ptr(ref.contiguous()) if R else None, H.ptr(n_ref.contiguous()), H.ptr(hyp.contiguous()) if Hn else None,
                                     H.ptr(n_hyp.contiguous()), H.ptr(counts), B, R, Hn, H.stream()))
    return counts


class _UCTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, n_steps, labels, n_labels):
        loss, status, grad = uctc_loss_and_grad(logits, n_steps, labels, n_labels)    # one launch gives both
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    def backward(ctx, g, _):
        grad, = ctx.saved_tensors
        return grad * g.float()[:, None, None], None, None, None


def uctc_loss(logits, n_steps, labels, n_labels):
    ''' the CTC objective as `F.ctc_loss(..., reduction='mean')` states it, differentiable in logits: -log p(labels | logits) of
        every row divided by its label count (at least 1), averaged over the rows with status 0.  Returns (that mean, the number of
        rows with another status -- no path, no step, a label out of range -- which contribute nothing) '''
    loss, status = _UCTC.apply(logits, n_steps, labels, n_labels)
    ok = status == 0
    per_label = torch.where(ok, loss / n_labels.clamp(min=1).to(loss.dtype), torch.zeros_like(loss))
    return per_label.sum() / ok.sum().clamp(min=1).to(loss.dtype), (~ok).sum()


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

def stress_fold(symbols):
    ''' the default `fold` of `phone_error_rates`: a class map (V,) int64 that sends every phone of the table to the first phone
        with the same name once a trailing stress digit is dropped (AH0, AH1, AH2 -> the class of AH0); the blank stays 0 '''
    phones = phones_of(symbols)
    first = {}
    fold = [0]
    for i, p in enumerate(phones):
        fold.append(first.setdefault(p.rstrip('012'), i + 1))
    return torch.tensor(fold, dtype=torch.int64)


class Recognizer(nn.Module):
    ''' the natural-log mel (B, n_mel, T), normalised per utterance and channel to zero mean and unit variance over its live
        frames -> `stride` adjacent frames stacked (n_steps = ceil(n_frames / stride)) -> `layers` x (Conv1d(3) -> ReLU), masked at
        the sequence end in front of every convolution -> Linear to 1 + len(phones) classes: class 0 the blank, class c the phone
        `phones[c - 1]`, the phones being `g2p.phones_of(symbols)` (pad, eos, whitespace and punctuation are not classes) '''
    def __init__(self, symbols, n_mel, hidden=256, layers=3, stride=2):
        super().__init__()
        assert int(layers) >= 1 and int(stride) >= 1
        self.args = dict(symbols=list(symbols), n_mel=int(n_mel), hidden=int(hidden), layers=int(layers), stride=int(stride))
        self.symbols, self.phones, self.stride, self.n_mel = list(symbols), phones_of(symbols), int(stride), int(n_mel)
        index = {p: i + 1 for i, p in enumerate(self.phones)}
        self.register_buffer('class_of', torch.tensor([index.get(s, 0) for s in self.symbols], dtype=torch.int64), persistent=False)
        widths = [self.n_mel * self.stride] + [int(hidden)] * int(layers)
        self.convs = nn.ModuleList(nn.Conv1d(a, b, 3, padding=1) for a, b in zip(widths[:-1], widths[1:]))
        self.out = nn.Linear(int(hidden), 1 + len(self.phones))

    def n_steps_of(self, n_frames):
        ''' ceil(n_frames / stride) '''
        return (n_frames + (self.stride - 1)) // self.stride

    def normalise(self, mel, n_frames):
        ''' (B, n_mel, T) -> time-major (B, T, n_mel) fp32: per utterance and channel, mean 0 and variance 1 over the frames below
            n_frames (a decoder's mel and a re-analysed waveform land in the same range); 0 at and past n_frames, whatever was there '''
        live = (torch.arange(mel.shape[2], device=mel.device)[None] < n_frames[:, None])[:, :, None]
        x = torch.where(live, mel.float().transpose(1, 2), torch.zeros((), dtype=torch.float32, device=mel.device))
        n = n_frames.clamp(min=1).to(torch.float32)[:, None, None]
        mean = x.sum(dim=1, keepdim=True) / n
        centred = torch.where(live, x - mean, torch.zeros_like(x))
        var = (centred * centred).sum(dim=1, keepdim=True) / n
        return centred * torch.rsqrt(var + 1e-5)

    def forward(self, mel, n_frames):
        ''' mel (B, n_mel, T) natural-log, n_frames (B,) int64 -> (logits (B, ceil(T / stride), V) fp32 contiguous, n_steps (B,)) '''
        x = self.normalise(mel, n_frames)
        B, T, _ = x.shape
        Ts = (T + self.stride - 1) // self.stride
        x = F.pad(x, (0, 0, 0, Ts * self.stride - T)).reshape(B, Ts, self.stride * self.n_mel)
        n_steps = self.n_steps_of(n_frames)
        m = (torch.arange(Ts, device=x.device)[None] < n_steps[:, None]).to(torch.float32)[:, :, None]
        h = x
        for conv in self.convs:
            h = torch.relu(_conv(h * m, conv))
        return self.out(h).float().contiguous(), n_steps.contiguous()

    def labels_of(self, symbols, input_lengths):
        ''' symbol ids (B, L) int64 with their counts (B,) -> (labels (B, L) int64: the class ids of the phones among the first
            input_lengths[b] symbols, in order, the non-phones dropped, zeros behind; n_labels (B,) int64) '''
        B, L = symbols.shape
        live = torch.arange(L, device=symbols.device)[None] < input_lengths[:, None]
        cls = self.class_of.to(symbols.device)[symbols.clamp(0, len(self.symbols) - 1)] * live
        keep = cls > 0
        pos = torch.where(keep, torch.cumsum(keep, dim=1) - 1, torch.full_like(cls, L))      # the dropped go to a spare column
        labels = torch.zeros((B, L + 1), dtype=torch.int64, device=symbols.device).scatter_(1, pos, cls)
        return labels[:, :L].contiguous(), keep.sum(dim=1)

    def decode(self, mel, n_frames):
        ''' greedy decode: (ids (B, steps) int32 class ids, n_out (B,) int32) '''
        with torch.no_grad():
            ids, n_out, _ = uctc_greedy(*self(mel, n_frames))
        return ids, n_out


def phone_error_rates(recognizer, mel, n_frames, symbols, input_lengths, fold=None):
    ''' mel (B, n_mel, T) natural-log with n_frames (B,), against the symbol ids (B, L) / input_lengths (B,) that were asked for.
        One pass of the recogniser, `dx_uctc_greedy`, `dx_edit_distance`.  Returns {key: (B,) device tensor} for PER_KEYS: `sub`,
        `del`, `ins` (int32) of the cheapest alignment of the decode with the phones of the text, `n_ref` (phones of the text),
        `per` = (sub + del + ins) / n_ref (fp32, NaN for n_ref = 0) and `n_hyp` (phones decoded).  `fold`: a class map (V,) int64
        applied to both sides before the distance, e.g. `stress_fold(symbols)`; None compares the classes as they are. '''
    H.require_gpu(mel, n_frames, symbols, input_lengths)
    ids, n_out = recognizer.decode(mel, n_frames.long())
    with torch.no_grad():
        ref, n_ref = recognizer.labels_of(symbols.long(), input_lengths.long())
        hyp = ids.long()
        if fold is not None:
            fold = fold.to(hyp.device)
            ref, hyp = fold[ref], fold[hyp]
        counts = edit_distance(ref.to(torch.int32), n_ref, hyp.to(torch.int32), n_out.long())
        errors = counts[:, :3].sum(dim=1)
        per = torch.where(n_ref > 0, errors.float() / n_ref.clamp(min=1).float(), torch.full_like(errors, float('nan'), dtype=torch.float32))
    return dict(zip(PER_KEYS, (counts[:, 0], counts[:, 1], counts[:, 2], n_ref.to(torch.int32), per, n_out)))


def audio_error_rates(recognizer, wavs, n_samples, symbols, input_lengths, hparams, fold=None):
    ''' `phone_error_rates` of waveforms: wavs (B, S) fp32 / n_samples (B,) int64 on the device are analysed with
        `mel_spectrogram_batch`.  The front end's reflect padding needs more than half a window of samples: a shorter row (an empty
        synthesis) is not analysed and keeps 0 frames -- all its phones count as deleted. '''
    from daft_exprt.extract_features import mel_spectrogram_batch
    H.require_gpu(wavs, n_samples)
    B, dev = wavs.shape[0], wavs.device
    rows = torch.nonzero(n_samples > int(hparams.filter_length) // 2).flatten()
    mel = torch.zeros((B, int(hparams.n_mel_channels), 1), dtype=torch.float32, device=dev)
    n_frames = torch.zeros((B,), dtype=torch.int64, device=dev)
    if rows.numel():
        sub_mel, _, sub_n = mel_spectrogram_batch(wavs[rows].contiguous(), n_samples[rows].contiguous(), hparams)
        mel = torch.zeros((B, sub_mel.shape[1], sub_mel.shape[2]), dtype=torch.float32, device=dev)
        mel[rows], n_frames[rows] = sub_mel.float(), sub_n.long()
    return phone_error_rates(recognizer, mel, n_frames, symbols, input_lengths, fold)


def per_to_host(scores):
    ''' {key: list} of `phone_error_rates`' result, for a report '''
    return {key: scores[key].cpu().tolist() for key in PER_KEYS}


# ---- training and checkpoints ----------------------------------------------------------------------------------------------------------

def save_recognizer(recognizer, path):
    ''' the weights and the constructor arguments (the symbol table among them) '''
    torch.save({'args': dict(recognizer.args), 'state_dict': {k: v.detach().cpu() for k, v in recognizer.state_dict().items()}}, path)


def load_recognizer(path, device='cuda:0'):
    chk = torch.load(path, map_location='cpu')
    recognizer = Recognizer(**chk['args'])
    recognizer.load_state_dict(chk['state_dict'])
    return recognizer.to(H.device(device)).eval()


def _repeats(labels):
    return sum(1 for u in range(1, len(labels)) if labels[u] == labels[u - 1])


def read_items(list_file, hparams, device, batch_size=64):
    ''' [(symbol ids (L,) int64, mel (n_mel, T) fp32, name)] on the device, in the list's order: the `features_dir|feature_file|
        speaker_id` list read once through `DaftExprtDataLoader` and its collate, batch_size utterances per copy '''
    from daft_exprt.data_loader import DaftExprtDataCollate, DaftExprtDataLoader
    dataset, collate = DaftExprtDataLoader(list_file, hparams, shuffle=False), DaftExprtDataCollate(hparams)
    items = {}
    for start in range(0, len(dataset), int(batch_size)):
        rows = list(range(start, min(len(dataset), start + int(batch_size))))
        batch = collate([dataset[i] for i in rows])
        symbols, mel = batch[0].to(device), batch[8].to(device)
        for row, (n_sym, n_frm, feature_dir, feature_file) in enumerate(zip(batch[5].tolist(), batch[9].tolist(), batch[11], batch[12])):
            items[(feature_dir, feature_file)] = (symbols[row, :n_sym].clone(), mel[row, :, :n_frm].float().clone(), feature_file)
    return [items[(line[0], line[1])] for line in dataset.data]          # (the collate sorts a batch by length)


def collate_items(items, device):
    ''' [(ids, mel, ...)] -> symbols (B, L) int64, input_lengths (B,), mel (B, n_mel, T) fp32, n_frames (B,), zero-padded '''
    B, L, T = len(items), max(1, max(len(i[0]) for i in items)), max(1, max(i[1].shape[1] for i in items))
    symbols = torch.zeros((B, L), dtype=torch.int64, device=device)
    mel = torch.zeros((B, items[0][1].shape[0], T), dtype=torch.float32, device=device)
    for b, item in enumerate(items):
        symbols[b, :len(item[0])], mel[b, :, :item[1].shape[1]] = item[0], item[1]
    n_sym = torch.tensor([len(i[0]) for i in items], dtype=torch.int64, device=device)
    n_frm = torch.tensor([i[1].shape[1] for i in items], dtype=torch.int64, device=device)
    return symbols, n_sym, mel, n_frm


def corpus_rates(recognizer, items, device, fold=None, batch_size=64, decodes=0):
    ''' over a list of items: (summed errors / summed reference length or None without a reference phone, the summed sub, del,
        ins, n_ref, and up to `decodes` of (name, reference phones, decoded phones)) '''
    totals, shown = [0, 0, 0, 0], []
    max_t = limits()[0] * recognizer.stride
    items = [i for i in items if i[1].shape[1] <= max_t]
    for start in range(0, len(items), int(batch_size)):
        chunk = items[start: start + int(batch_size)]
        symbols, n_sym, mel, n_frm = collate_items(chunk, device)
        host = per_to_host(phone_error_rates(recognizer, mel, n_frm, symbols, n_sym, fold))
        for k, key in enumerate(('sub', 'del', 'ins', 'n_ref')):
            totals[k] += sum(host[key])
        if len(shown) < decodes:
            ids, n_out = recognizer.decode(mel, n_frm)
            ref, n_ref = recognizer.labels_of(symbols, n_sym)
            ids, n_out, ref, n_ref = ids.cpu().tolist(), n_out.cpu().tolist(), ref.cpu().tolist(), n_ref.cpu().tolist()
            for b, item in enumerate(chunk[: decodes - len(shown)]):
                name = item[2] if len(item) > 2 else str(start + b)
                shown.append((name, [recognizer.phones[c - 1] for c in ref[b][:n_ref[b]]],
                              [recognizer.phones[c - 1] for c in ids[b][:n_out[b]]]))
    rate = sum(totals[:3]) / totals[3] if totals[3] else None
    return rate, totals, shown


def train_recognizer(hparams, training_files, validation_files, steps=2000, batch_size=32, lr=1e-3, seed=1234, hidden=256, layers=3,
                     stride=2, log_every=100, device='cuda:0'):
    ''' trains a `Recognizer` on the utterances a `features_dir|feature_file|speaker_id` list names and returns (the model, a
        report).  Mels and symbols are read once through the data loader and its collate (`read_items`) and kept on the device;
        every step takes the next batch_size of a seeded permutation (one per epoch), Adam at `lr`.  Utterances beyond the limits of
        K31 (`limits()`: steps = ceil(frames / stride), phones, classes), without a phone, or with fewer steps than phones + equal
        neighbours (no CTC path) are left out and counted.
        The report: utterances_train, utterances_held_out, left_out, steps, loss (the last step's), skipped_rows (rows of all steps
        with a status other than 0: none is expected after the filter), phone_error_rate and phone_error_rate_folded (stress folded,
        `stress_fold`) on validation_files -- summed errors / summed reference length, None without a reference phone --, errors
        (the summed sub, del, ins, n_ref, unfolded) and held_out_decodes: up to 20 of (name, reference phones, decode). '''
    dev = H.device(device)
    max_t, max_u, max_v = limits()
    torch.manual_seed(int(seed))
    recognizer = Recognizer(hparams.symbols, int(hparams.n_mel_channels), hidden, layers, stride).to(dev)
    if 1 + len(recognizer.phones) > max_v:
        raise ValueError(f'train_recognizer: {len(recognizer.phones)} phones + blank exceed the {max_v} classes of the CTC kernels')
    class_of = recognizer.class_of.cpu().tolist()

    def usable(item):
        labels = [class_of[s] for s in item[0].cpu().tolist() if class_of[s] > 0]
        n_steps = (item[1].shape[1] + int(stride) - 1) // int(stride)
        return 0 < len(labels) <= max_u and n_steps <= max_t and n_steps >= len(labels) + _repeats(labels)

    read = read_items(training_files, hparams, dev)
    items = [item for item in read if usable(item)]
    left_out = len(read) - len(items)
    if not items:
        raise ValueError('train_recognizer: no utterance to train on')
    held = read_items(validation_files, hparams, dev) if validation_files else []
    _logger.info(f'train_recognizer: {len(items)} utterances on the device, {left_out} left out, {len(held)} held out')
    recognizer.train()
    optimizer = torch.optim.Adam(recognizer.parameters(), lr=float(lr))
    gen = torch.Generator().manual_seed(int(seed))
    skipped_rows = torch.zeros((), dtype=torch.int64, device=dev)
    loss, order = None, []
    for step in range(int(steps)):
        if len(order) < min(int(batch_size), len(items)):
            order = torch.randperm(len(items), generator=gen).tolist()
        idx, order = order[:int(batch_size)], order[int(batch_size):]
        symbols, n_sym, mel, n_frm = collate_items([items[i] for i in idx], dev)
        labels, n_labels = recognizer.labels_of(symbols, n_sym)
        logits, n_steps = recognizer(mel, n_frm)
        loss, skipped = uctc_loss(logits, n_steps, labels[:, :max_u].contiguous(), n_labels)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        skipped_rows += skipped
        if log_every and (step % int(log_every) == 0 or step == int(steps) - 1):
            _logger.info(f'train_recognizer: step {step} -- CTC loss per phone {float(loss.detach()):.5f} -- rows without a path so far '
                         f'{int(skipped_rows)}')
    recognizer.eval()
    report = dict(utterances_train=len(items), utterances_held_out=len(held), left_out=left_out, steps=int(steps),
                  loss=float(loss.detach()) if loss is not None else None, skipped_rows=int(skipped_rows), phone_error_rate=None,
                  phone_error_rate_folded=None, errors=None, held_out_decodes=[])
    if held:
        rate, totals, shown = corpus_rates(recognizer, held, dev, decodes=20)
        folded, _, _ = corpus_rates(recognizer, held, dev, fold=stress_fold(hparams.symbols))
        report.update(phone_error_rate=rate, phone_error_rate_folded=folded, errors=dict(zip(('sub', 'del', 'ins', 'n_ref'), totals)),
                      held_out_decodes=shown)
    return recognizer, report
