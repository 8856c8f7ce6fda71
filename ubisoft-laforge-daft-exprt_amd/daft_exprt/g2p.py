"""Grapheme-to-phoneme conversion learned from the user's own pronunciation dictionary on the GPU.

The reference sends every word its dictionary lacks to `mfa g2p` (`generate.py:84-105`).  Here a small non-autoregressive model is
trained on the dictionary itself: a grapheme encoder, `expand` output slots per grapheme, a softmax over the phones plus a blank,
and the CTC loss; decoding is greedy.  The lattice work -- the CTC loss with its gradient (`ctc_loss`) and the greedy decode
(`ctc_greedy`) -- are the kernels of csrc/g2p.hip (K30); the encoder is plain torch (plumbing, as in `aligner.Aligner`).
`train_g2p` trains one on a dictionary as `text.load_dictionary` returns it, `G2P.phonemize` transcribes words, and
`scripts/train_g2p.py` / `scripts/phonemize.py` are the command lines.

The arithmetic is pinned against tests/ctc_oracle.py.  How accurate such a model is on a real dictionary such as CMUdict has NOT
been measured: no accuracy on English is claimed.  No CPU fallback: without the HIP library / a GPU the device functions raise.
"""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H

_logger = logging.getLogger(__name__)

GRAPHEMES = "abcdefghijklmnopqrstuvwxyz'"       # the reference's word pattern is [\w']+ on cleaned (ASCII, lower-case) text; id 0 pads


def limits():
    ''' (steps, labels, classes): the largest T, U and V (blank included) the K30 kernels admit '''
    lib = H.lib()
    return int(lib.dx_ctc_max_steps()), int(lib.dx_ctc_max_labels()), int(lib.dx_ctc_max_classes())


def phones_of(symbols):
    ''' the phones of a symbol table (`hparams.symbols`): everything but pad, eos, whitespace and punctuation, in table order '''
    from daft_exprt.symbols import eos, pad, punctuation, whitespace
    other = set(pad + eos + whitespace + punctuation)
    return [s for s in symbols if s not in other]


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------

def _check_logits(who, logits, n_steps, U=0):
    H.require_gpu(logits, n_steps)
    assert logits.dtype == torch.float32 and logits.dim() == 3 and n_steps.dtype == torch.int64 and n_steps.shape == (logits.shape[0],)
    B, T, V = logits.shape
    max_t, max_u, max_v = limits()
    if T > max_t or U > max_u or V > max_v:
        raise ValueError(f'{who}: {T} steps (at most {max_t}), {U} labels (at most {max_u}) or {V} classes (at most {max_v})')
    return logits.contiguous(), n_steps.contiguous()


def ctc_loss_and_grad(logits, n_steps, labels, n_labels, w=None):
    ''' `dx_ctc_loss`: logits (B, T, V) fp32, labels (B, U) int64 in [1, V - 1], w (B,) fp32 (default: ones) ->
        (loss (B,) fp32, status (B,) int32, grad (B, T, V) fp32 = w[b] dloss[b] / dlogits); blank is class 0 '''
    H.require_gpu(labels, n_labels)
    B, T, V = logits.shape
    assert labels.dtype == torch.int64 and labels.dim() == 2 and labels.shape[0] == B and n_labels.dtype == torch.int64 and n_labels.shape == (B,)
    U = labels.shape[1]
    logits, n_steps = _check_logits('ctc_loss', logits, n_steps, U)
    dev = logits.device
    w = torch.ones((B,), dtype=torch.float32, device=dev) if w is None else w.float().contiguous()
    assert w.shape == (B,)
    loss = torch.empty((B,), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    grad = torch.empty_like(logits)
    ws = torch.empty((B, T, 2 * U + 1), dtype=torch.float32, device=dev)
    H.check(H.lib().dx_ctc_loss(H.ptr(logits), H.ptr(n_steps), H.ptr(labels.contiguous()) if U else None, H.ptr(n_labels.contiguous()),
                                H.ptr(w), H.ptr(loss), H.ptr(status), H.ptr(grad), H.ptr(ws), B, T, U, V, H.stream()))
    return loss, status, grad


def ctc_greedy(logits, n_steps):
    ''' `dx_ctc_greedy`: -> (ids (B, T) int32: the arg-max path with repeats collapsed and blanks dropped, zeros behind n_out;
        n_out (B,) int32; score (B,) fp32: the summed log-probability of the arg-max path) '''
    logits, n_steps = _check_logits('ctc_greedy', logits, n_steps)
    B, T, V = logits.shape
    ids = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    n_out = torch.empty((B,), dtype=torch.int32, device=logits.device)
    score = torch.empty((B,), dtype=torch.float32, device=logits.device)
    H.check(H.lib().dx_ctc_greedy(H.ptr(logits), H.ptr(n_steps), H.ptr(ids), H.ptr(n_out), H.ptr(score), B, T, V, H.stream()))
    return ids, n_out, score


class _CTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, n_steps, labels, n_labels):
        loss, status, grad = ctc_loss_and_grad(logits, n_steps, labels, n_labels)     # one launch gives both
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(status)
        return loss, status

    @staticmethod
    def backward(ctx, g, _):
        grad, = ctx.saved_tensors
        return grad * g.float()[:, None, None], None, None, None


def ctc_loss(logits, n_steps, labels, n_labels):
    ''' the CTC objective, differentiable in logits: returns (mean of -log p(labels | logits) over the rows with status 0, the
        number of rows with another status -- no path, no step, a label out of range -- which contribute nothing) '''
    loss, status = _CTC.apply(logits, n_steps, labels, n_labels)
    ok = status == 0
    return torch.where(ok, loss, torch.zeros_like(loss)).sum() / ok.sum().clamp(min=1).to(loss.dtype), (~ok).sum()


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

def _conv(x, conv):
    ''' a Conv1d (odd kernel, same padding) over time-major x (B, N, C) as one matrix product over the stacked taps '''
    w = conv.weight
    k = w.shape[2]
    if k == 1:
        return F.linear(x, w[:, :, 0], conv.bias)
    pad = F.pad(x, (0, 0, k // 2, k // 2))
    taps = torch.cat([pad[:, i: i + x.shape[1]] for i in range(k)], dim=2)
    return F.linear(taps, w.permute(0, 2, 1).reshape(w.shape[0], -1), conv.bias)


class G2P(nn.Module):
    ''' embedding -> `layers` x (Conv1d(kernel) -> ReLU) at the grapheme rate, masked at the word's end in front of every
        convolution (receptive field +- layers * (kernel // 2) graphemes: +- 4 by default, a final silent `e` acts two letters
        back) -> Linear to `expand` slots per grapheme -> ReLU -> Linear to 1 + len(phones) classes, class 0 the blank '''
    def __init__(self, phones, hidden=128, expand=3, layers=2, kernel=5, graphemes=GRAPHEMES):
        super().__init__()
        assert int(kernel) % 2 == 1 and int(layers) * (int(kernel) // 2) >= 4, 'the receptive field must cover +- 4 graphemes'
        self.args = dict(phones=list(phones), hidden=int(hidden), expand=int(expand), layers=int(layers), kernel=int(kernel),
                         graphemes=str(graphemes))
        self.phones, self.graphemes, self.expand_by, self.hidden = list(phones), str(graphemes), int(expand), int(hidden)
        self.embedding = nn.Embedding(len(self.graphemes) + 1, hidden)
        self.convs = nn.ModuleList(nn.Conv1d(hidden, hidden, int(kernel), padding=int(kernel) // 2) for _ in range(int(layers)))
        self.expand = nn.Linear(hidden, self.expand_by * hidden)
        self.out = nn.Linear(hidden, 1 + len(self.phones))

    def grapheme_ids(self, word):
        ''' the ids of a word's characters (lower-cased), or None when one is outside the grapheme table '''
        ids = [self.graphemes.find(c) + 1 for c in word.lower()]
        return ids if ids and all(ids) else None

    def forward(self, graphemes, n_graphemes):
        ''' graphemes (B, L) int64 (0 pads), n_graphemes (B,) int64 -> (logits (B, L * expand, V) fp32 contiguous, n_steps (B,)) '''
        m = (torch.arange(graphemes.shape[1], device=graphemes.device)[None] < n_graphemes[:, None]).to(torch.float32)[:, :, None]
        h = self.embedding(graphemes) * m
        for conv in self.convs:
            h = torch.relu(_conv(h, conv)) * m
        y = torch.relu(self.expand(h)).reshape(graphemes.shape[0], graphemes.shape[1] * self.expand_by, self.hidden)
        return self.out(y).float().contiguous(), (n_graphemes * self.expand_by).contiguous()

    def phonemize(self, words, batch_size=1024):
        ''' [phones or None] for the words, in their order: batches of batch_size words sorted by length, one pass of the encoder
            and one `dx_ctc_greedy` per batch.  None for a word whose decode is empty, which holds a character outside the
            grapheme table, or which is too long for the kernel (len * expand > `limits()[0]`). '''
        dev = self.out.weight.device
        max_t = limits()[0]
        out = [None] * len(words)
        todo = [(i, ids) for i, ids in ((i, self.grapheme_ids(w)) for i, w in enumerate(words))
                if ids is not None and len(ids) * self.expand_by <= max_t]
        todo.sort(key=lambda item: len(item[1]))
        was_training = self.training
        self.eval()
        with torch.no_grad():
            for pos in range(0, len(todo), int(batch_size)):
                chunk = todo[pos: pos + int(batch_size)]
                L = len(chunk[-1][1])
                g = torch.tensor([ids + [0] * (L - len(ids)) for _, ids in chunk], dtype=torch.int64, device=dev)
                n = torch.tensor([len(ids) for _, ids in chunk], dtype=torch.int64, device=dev)
                ids, n_out, _ = ctc_greedy(*self(g, n))
                ids, n_out = ids.cpu().tolist(), n_out.cpu().tolist()
                for row, (i, _) in enumerate(chunk):
                    if n_out[row] > 0:
                        out[i] = [self.phones[c - 1] for c in ids[row][:n_out[row]]]
        self.train(was_training)
        return out


# ---- training and checkpoints ----------------------------------------------------------------------------------------------------------

def save_g2p(g2p, path):
    ''' the weights and the constructor arguments (the phone and grapheme tables among them) '''
    torch.save({'args': dict(g2p.args), 'state_dict': {k: v.detach().cpu() for k, v in g2p.state_dict().items()}}, path)


def load_g2p(path, device='cuda:0'):
    chk = torch.load(path, map_location='cpu')
    g2p = G2P(**chk['args'])
    g2p.load_state_dict(chk['state_dict'])
    return g2p.to(H.device(device)).eval()


def _edit_distance(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[len(b)]


def error_rates(decodes, references):
    ''' decodes: [phones or None]; references: [[pronunciation, ...]] per word.  Returns (phone error rate: the summed edit distance
        to the closest listed pronunciation / the summed length of that pronunciation, a None decode counting as empty;  word error
        rate: the share of words whose decode equals none of the listed pronunciations) '''
    dist = length = wrong = 0
    for decode, prons in zip(decodes, references):
        d, n = min((_edit_distance(decode or [], p), len(p)) for p in prons)
        dist, length, wrong = dist + d, length + n, wrong + (decode not in prons)
    return dist / max(1, length), wrong / max(1, len(references))


def length_sorted_batches(lengths, batch_size, generator):
    ''' endless batches of indices into the packed lexicon: ONE seeded permutation of the N pairs per epoch, cut into slices of
        batch_size (the last of an epoch may be shorter), each slice sorted by length.  Yields (indices (b,) int64 on the host, the
        largest length among them).  Per step the host touches batch_size numbers, not N. '''
    lengths = torch.as_tensor(lengths, dtype=torch.int64)
    while True:
        perm = torch.randperm(len(lengths), generator=generator)
        for pos in range(0, len(lengths), int(batch_size)):
            idx = perm[pos: pos + int(batch_size)]
            idx = idx[torch.argsort(lengths[idx], stable=True)]
            yield idx, int(lengths[idx[-1]])


def train_g2p(dictionary, hparams, steps=5000, batch_size=256, lr=2e-3, seed=1234, held_out=0.05, hidden=128, expand=3, layers=2,
              kernel=5, log_every=500, device='cuda:0'):
    ''' trains a `G2P` on a pronunciation dictionary -- `{word: [phones, ...]}` as `text.load_dictionary` returns it, or the path
        of one -- and returns (the model, a report).  Every pronunciation of every word is a training pair.  The WORDS are split by
        a seeded permutation: round(held_out * words) of them are held out with all their pronunciations.  The training pairs are
        packed once on the device as id tensors; every step takes the next batch_size of a seeded permutation (one per epoch,
        `length_sorted_batches`), sorted by length so the waves of a workgroup of K30 end together, Adam at `lr`.  A phone outside
        `hparams.symbols` raises ValueError naming the word.  Words with a character outside the grapheme table,
        and pairs beyond the kernel's limits, are left out and counted.
        The report: words_train, words_held_out, pairs_train, left_out, steps, loss (the last step's), skipped_rows (rows of all
        steps without a CTC path: fewer output slots than phones + equal neighbours), phone_error_rate and word_error_rate on the
        held-out words (`error_rates`; None without held-out words) and held_out_decodes: up to 20 of (word, decode, listed). '''
    if not isinstance(dictionary, dict):
        from daft_exprt.text import load_dictionary
        dictionary = load_dictionary(dictionary, hparams.symbols)
    dev = H.device(device)
    phones = phones_of(hparams.symbols)
    max_t, max_u, max_v = limits()
    if 1 + len(phones) > max_v:
        raise ValueError(f'train_g2p: {len(phones)} phones + blank exceed the {max_v} classes of the CTC kernels')
    index = {p: i + 1 for i, p in enumerate(phones)}
    for word, prons in dictionary.items():
        unknown = [p for pron in prons for p in pron if p not in index]
        if unknown:
            raise ValueError(f'train_g2p: unknown phone "{unknown[0]}" in the pronunciation of "{word}"')
    torch.manual_seed(int(seed))
    g2p = G2P(phones, hidden, expand, layers, kernel).to(dev)
    words = sorted(w for w in dictionary if g2p.grapheme_ids(w) is not None)
    left_out = len(dictionary) - len(words)
    gen = torch.Generator().manual_seed(int(seed))
    order = torch.randperm(len(words), generator=gen).tolist()
    n_held = int(round(float(held_out) * len(words)))
    held = [words[i] for i in order[:n_held]]
    pairs = []
    for i in order[n_held:]:
        for pron in dictionary[words[i]]:
            if pron and len(words[i]) * int(expand) <= max_t and len(pron) <= max_u:
                pairs.append((g2p.grapheme_ids(words[i]), [index[p] for p in pron]))
            else:
                left_out += 1
    if not pairs:
        raise ValueError('train_g2p: no pronunciation to train on')
    N, L, U = len(pairs), max(len(g) for g, _ in pairs), max(len(p) for _, p in pairs)
    lengths = [len(g) for g, _ in pairs]
    graphemes = torch.tensor([g + [0] * (L - len(g)) for g, _ in pairs], dtype=torch.int64).to(dev)
    labels = torch.tensor([p + [0] * (U - len(p)) for _, p in pairs], dtype=torch.int64).to(dev)
    n_graphemes = torch.tensor(lengths, dtype=torch.int64).to(dev)
    n_labels = torch.tensor([len(p) for _, p in pairs], dtype=torch.int64).to(dev)
    _logger.info(f'train_g2p: {N} pairs of {len(words) - n_held} words on the device, {n_held} words held out, {left_out} left out')
    g2p.train()
    optimizer = torch.optim.Adam(g2p.parameters(), lr=float(lr))
    skipped_rows = torch.zeros((), dtype=torch.int64, device=dev)
    loss = None
    batches = length_sorted_batches(lengths, batch_size, gen)
    for step in range(int(steps)):
        idx, Lb = next(batches)
        idx = idx.to(dev)
        nl = n_labels[idx]
        logits, n_steps = g2p(graphemes[idx, :Lb].contiguous(), n_graphemes[idx])
        loss, skipped = ctc_loss(logits, n_steps, labels[idx].contiguous(), nl.contiguous())
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        skipped_rows += skipped
        if log_every and (step % int(log_every) == 0 or step == int(steps) - 1):
            _logger.info(f'train_g2p: step {step} -- CTC loss per word {float(loss.detach()):.5f} -- rows without a path so far '
                         f'{int(skipped_rows)}')
    g2p.eval()
    report = dict(words_train=len(words) - n_held, words_held_out=n_held, pairs_train=N, left_out=left_out, steps=int(steps),
                  loss=float(loss.detach()) if loss is not None else None, skipped_rows=int(skipped_rows), phone_error_rate=None,
                  word_error_rate=None, held_out_decodes=[])
    if held:
        decodes = g2p.phonemize(held)
        report['phone_error_rate'], report['word_error_rate'] = error_rates(decodes, [dictionary[w] for w in held])
        report['held_out_decodes'] = [(w, d, dictionary[w]) for w, d in list(zip(held, decodes))[:20]]
    return g2p, report
