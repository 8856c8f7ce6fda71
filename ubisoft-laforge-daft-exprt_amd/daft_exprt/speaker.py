"""Speaker identity: a speaker encoder trained on the corpus's own feature files, and the scores that say whose voice a synthesis
has, on the GPU.  The reference has no counterpart.

Daft-Exprt trains an adversarial speaker classifier so that the prosody encoder's FiLM vectors carry the reference's prosody and
not its speaker; nothing measured whether the output sounds like the requested speaker or whether the reference's speaker leaks
through.  Here a small convolutional encoder over the natural-log mel -- level removed by ONE scalar mean and variance per utterance,
the spectral shape kept -- pools its frames with attentive statistics (`attn_stat_pool`) into a unit-length embedding and is trained
with an additive-margin softmax over the corpus's speakers.  A synthesis is scored by the cosine of its embedding to the centroid
of the requested speaker, to the other centroids and to the embedding of the prosody reference (`speaker_scores`); the encoder's own
quality is the identification error and the equal error rate over all held-out verification trials (`trial_counts`,
`eer_from_counts`).  The pooling with its backward and the trial histograms are the kernels of csrc/speaker.hip (K32); the encoder is
plain torch (plumbing, as in `recognizer.Recognizer`).  `train_speaker_encoder` trains one from file lists, and
`scripts/train_speaker_encoder.py`, `scripts/evaluate.py -spk` and `scripts/synthesize.py -spk` are the command lines.

The arithmetic is pinned against tests/speaker_oracle.py.  What nobody has measured: the encoder's error rates on real speech, and
how its cosine scores track listeners' judgement of speaker similarity -- neither is claimed.  An encoder trained on a small corpus
errs on recordings too: read a synthesis's scores beside those of the recording (`evaluate.copy_synthesis_scores` reports both).
No CPU fallback: without the HIP library / a GPU the device functions raise.
"""
import logging
from fractions import Fraction

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from daft_exprt import _hip as H
from daft_exprt.g2p import _conv

_logger = logging.getLogger(__name__)

SPEAKER_KEYS = ('cos_target', 'margin', 'identified', 'accepted')      # `speaker_scores`; with reference embeddings also:
REFERENCE_KEY = 'cos_reference'
TRIAL_BINS = 4096                                                      # bins of `trial_counts` over cosines in [-1, 1]


def limits():
    ''' (channels, steps, dim, rows): the largest C and T `attn_stat_pool` admits, the largest D and N `trial_counts` admits '''
    lib = H.lib()
    return int(lib.dx_spk_pool_max_channels()), int(lib.dx_spk_pool_max_steps()), int(lib.dx_trial_max_dim()), int(lib.dx_trial_max_rows())


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------

def _check_pool(h, a, n_steps):
    H.require_gpu(h, a, n_steps)
    assert h.dtype == torch.float32 and h.dim() == 3 and a.dtype == torch.float32 and a.shape == h.shape[:2]
    assert n_steps.dtype == torch.int64 and n_steps.shape == (h.shape[0],)
    B, T, C = h.shape
    max_c, max_t, _, _ = limits()
    if C > max_c or T > max_t or min(B, T, C) < 1:
        raise ValueError(f'attn_stat_pool: {C} channels (at most {max_c}) or {T} steps (at most {max_t}), at least one row, step and channel')


def attn_stat_pool_forward(h, a, n_steps):
    ''' `dx_attn_stat_pool_fwd`: h (B, T, C) fp32 time-major, a (B, T) fp32 logits, n_steps (B,) int64 -> (out (B, 2 C) = [mu, sd]
        of the softmax(a)-weighted frames below n_steps, stat (B, 2): the softmax's max and normaliser) '''
    _check_pool(h, a, n_steps)
    B, T, C = h.shape
    h, a, n_steps = h.contiguous(), a.contiguous(), n_steps.contiguous()
    out = torch.empty((B, 2 * C), dtype=torch.float32, device=h.device)
    stat = torch.empty((B, 2), dtype=torch.float32, device=h.device)
    H.check(H.lib().dx_attn_stat_pool_fwd(H.ptr(h), H.ptr(a), H.ptr(n_steps), H.ptr(out), H.ptr(stat), B, T, C, H.stream()))
    return out, stat


def attn_stat_pool_backward(h, a, n_steps, out, stat, g_out):
    ''' `dx_attn_stat_pool_bwd`: the inputs, outputs and g_out (B, 2 C) of the forward -> (g_h (B, T, C), g_a (B, T)) '''
    _check_pool(h, a, n_steps)
    H.require_gpu(out, stat, g_out)
    B, T, C = h.shape
    assert out.shape == (B, 2 * C) and stat.shape == (B, 2) and g_out.shape == (B, 2 * C)
    h, a, n_steps, g_out = h.contiguous(), a.contiguous(), n_steps.contiguous(), g_out.float().contiguous()
    g_h, g_a = torch.empty_like(h), torch.empty_like(a)
    ws = torch.empty((B, (C + 63) // 64, T), dtype=torch.float32, device=h.device)
    H.check(H.lib().dx_attn_stat_pool_bwd(H.ptr(h), H.ptr(a), H.ptr(n_steps), H.ptr(out.contiguous()), H.ptr(stat.contiguous()),
                                          H.ptr(g_out), H.ptr(g_h), H.ptr(g_a), H.ptr(ws), B, T, C, H.stream()))
    return g_h, g_a


class _AttnStatPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, a, n_steps):
        out, stat = attn_stat_pool_forward(h, a, n_steps)
        ctx.save_for_backward(h, a, n_steps, out, stat)
        return out

    @staticmethod
    def backward(ctx, g_out):
        g_h, g_a = attn_stat_pool_backward(*ctx.saved_tensors, g_out)
        return g_h, g_a, None


def attn_stat_pool(h, a, n_steps):
    ''' attentive statistics pooling, differentiable in h and a: (B, 2 C) = the mean and the standard deviation (about that mean,
        + 1e-5 under the root) of every channel over the live steps, weighted by softmax(a) over them; zeros for a row without steps '''
    return _AttnStatPool.apply(h, a, n_steps)


def trial_counts(E, spk):
    ''' `dx_trial_counts`: E (N, D) fp32 rows of unit length, spk (N,) int32 -> counts (2, 4096) int64: the histogram of the cosine
        of every unordered pair over bins of 2 / 4096, row 0 the pairs of one speaker (targets), row 1 the others (non-targets) '''
    H.require_gpu(E, spk)
    assert E.dtype == torch.float32 and E.dim() == 2 and spk.dtype == torch.int32 and spk.shape == (E.shape[0],)
    N, D = E.shape
    _, _, max_d, max_n = limits()
    if not (1 <= N <= max_n and 1 <= D <= max_d):
        raise ValueError(f'trial_counts: {N} rows (at most {max_n}) or {D} columns (at most {max_d}), at least one of each')
    E, spk = E.contiguous(), spk.contiguous()
    counts = torch.empty((2, TRIAL_BINS), dtype=torch.int64, device=E.device)
    H.check(H.lib().dx_trial_counts(H.ptr(E), H.ptr(spk), H.ptr(counts), N, D, H.stream()))
    return counts


def eer_from_counts(counts):
    ''' the equal error rate and its threshold from the (2, 4096) histograms of `trial_counts` (a tensor or an array), on the host.
        The threshold is the lower edge of bin k, k in 0 .. 4096, and a trial is accepted when its bin >= k:
          FAR_k = sum_{b >= k} non-targets / all non-targets,   FRR_k = sum_{b < k} targets / all targets;
        the rate is (FAR_k + FRR_k) / 2 at the k that minimises |FAR_k - FRR_k| (compared exactly, in integers; the lowest such k on
        a tie).  Returns (eer, threshold = k / 2048 - 1), or None when either class has no trial.  The resolution is the bin width:
        2 / 4096 in cosine. '''
    counts = counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    tar, non = counts[0].astype(np.int64), counts[1].astype(np.int64)
    n_tar, n_non = int(tar.sum()), int(non.sum())
    if n_tar == 0 or n_non == 0:
        return None
    rejected = np.concatenate([[0], np.cumsum(tar)])                  # targets in the bins below k
    accepted = n_non - np.concatenate([[0], np.cumsum(non)])         # non-targets in the bins at or above k
    k = int(np.argmin(np.abs(accepted * n_tar - rejected * n_non)))  # |FAR - FRR| n_tar n_non: below 2^62 at 65 536 rows
    eer = (Fraction(int(accepted[k]), n_non) + Fraction(int(rejected[k]), n_tar)) / 2                # rounded once
    return float(eer), k * 2.0 / TRIAL_BINS - 1.0


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

class SpeakerEncoder(nn.Module):
    ''' the natural-log mel (B, n_mel, T), normalised per utterance by ONE scalar mean and variance over all its live frames and
        channels (the level goes, the spectral shape -- what identifies a speaker -- stays; `Recognizer`'s per-channel statistics
        would remove it) -> `stride` adjacent frames stacked -> `layers` x (Conv1d(3) -> ReLU), masked at the sequence end in front of
        every convolution -> attention logits Linear(hidden, 64) -> tanh -> Linear(64, 1) -> `attn_stat_pool` -> Linear(2 hidden,
        dim).  `embed` returns rows of unit length.  After training the encoder carries `speaker_ids`, one `centroids` row per
        speaker, and the `threshold` and `eer` of its held-out trials (`set_speakers`). '''
    def __init__(self, n_mel, hidden=256, layers=3, stride=2, dim=128):
        super().__init__()
        assert int(layers) >= 1 and int(stride) >= 1 and int(dim) >= 1
        self.args = dict(n_mel=int(n_mel), hidden=int(hidden), layers=int(layers), stride=int(stride), dim=int(dim))
        self.n_mel, self.stride = int(n_mel), int(stride)
        widths = [self.n_mel * self.stride] + [int(hidden)] * int(layers)
        self.convs = nn.ModuleList(nn.Conv1d(a, b, 3, padding=1) for a, b in zip(widths[:-1], widths[1:]))
        self.att_in, self.att_out = nn.Linear(int(hidden), 64), nn.Linear(64, 1)
        self.out = nn.Linear(2 * int(hidden), int(dim))
        self.speaker_ids, self.threshold, self.eer = [], None, None
        self.register_buffer('centroids', torch.zeros((0, int(dim))), persistent=False)

    def set_speakers(self, speaker_ids, centroids, threshold=None, eer=None):
        ''' the corpus's speaker ids, their centroids (S, dim) of unit length in that order, the decision threshold and the EER '''
        assert len(speaker_ids) == centroids.shape[0] and centroids.shape[1] == self.args['dim']
        self.speaker_ids = [int(s) for s in speaker_ids]
        self.centroids = centroids.detach().to(self.out.weight.device, torch.float32)
        self.threshold = None if threshold is None else float(threshold)
        self.eer = None if eer is None else float(eer)

    def n_steps_of(self, n_frames):
        ''' ceil(n_frames / stride) '''
        return (n_frames + (self.stride - 1)) // self.stride

    def normalise(self, mel, n_frames):
        ''' (B, n_mel, T) -> time-major (B, T, n_mel) fp32 with mean 0 and variance 1 over ALL live entries of the utterance -- one
            scalar each, over frames and channels; 0 at and past n_frames, whatever was there '''
        live = (torch.arange(mel.shape[2], device=mel.device)[None] < n_frames[:, None])[:, :, None]
        x = torch.where(live, mel.float().transpose(1, 2), torch.zeros((), dtype=torch.float32, device=mel.device))
        n = (n_frames.clamp(min=1) * mel.shape[1]).to(torch.float32)[:, None, None]
        mean = x.sum(dim=(1, 2), keepdim=True) / n
        centred = torch.where(live, x - mean, torch.zeros_like(x))
        var = (centred * centred).sum(dim=(1, 2), keepdim=True) / n
        return centred * torch.rsqrt(var + 1e-5)

    def frames(self, mel, n_frames):
        ''' everything in front of the pooling: (h (B, steps, hidden) fp32 contiguous, a (B, steps) attention logits, n_steps (B,)) '''
        x = self.normalise(mel, n_frames)
        B, T, _ = x.shape
        Ts = (T + self.stride - 1) // self.stride
        x = F.pad(x, (0, 0, 0, Ts * self.stride - T)).reshape(B, Ts, self.stride * self.n_mel)
        n_steps = self.n_steps_of(n_frames)
        m = (torch.arange(Ts, device=x.device)[None] < n_steps[:, None]).to(torch.float32)[:, :, None]
        h = x
        for conv in self.convs:
            h = torch.relu(_conv(h * m, conv))
        h = h.float().contiguous()
        a = self.att_out(torch.tanh(self.att_in(h)))[:, :, 0].float().contiguous()
        return h, a, n_steps.contiguous()

    def forward(self, mel, n_frames):
        ''' mel (B, n_mel, T) natural-log, n_frames (B,) int64 -> the embedding (B, dim) before it is brought to unit length '''
        return self.out(attn_stat_pool(*self.frames(mel, n_frames)))

    def embed(self, mel, n_frames):
        ''' rows of unit length (B, dim) '''
        return F.normalize(self(mel, n_frames), dim=1)


def am_softmax_loss(embeddings, class_weights, targets, scale=30.0, margin=0.2):
    ''' the additive-margin softmax: unit embeddings (B, dim) against unit class weights (S, dim), `scale` (cos - margin onehot),
        then the cross entropy.  A few small matrix products at B x S: plain torch '''
    cos = F.normalize(embeddings, dim=1) @ F.normalize(class_weights, dim=1).t()
    return F.cross_entropy(float(scale) * (cos - float(margin) * F.one_hot(targets, cos.shape[1]).to(cos.dtype)), targets)


# ---- scoring -----------------------------------------------------------------------------------------------------------------------------

def speaker_scores(encoder, mel, n_frames, target_ids, reference_embeddings=None):
    ''' mel (B, n_mel, T) natural-log with n_frames (B,) against the speakers that were asked for: target_ids (B,), a tensor or a
        list of the corpus's speaker ids (`encoder.speaker_ids`).  One pass of the encoder.  Returns {key: (B,) device tensor}:
          cos_target   the cosine of the embedding to the centroid of the requested speaker (fp32)
          margin       cos_target minus the largest cosine to any OTHER centroid
          identified   the nearest centroid is the requested speaker's (bool)
          accepted     cos_target >= encoder.threshold (bool; False without a threshold)
          cos_reference (with `reference_embeddings` (B, dim), e.g. `encoder.embed` of the prosody references) the cosine to that
                       row's reference embedding.
        A row without frames, or whose speaker the encoder does not know, scores NaN and is neither identified nor accepted. '''
    H.require_gpu(mel, n_frames)
    assert len(encoder.speaker_ids) >= 2, 'speaker_scores: the encoder carries no centroids (train_speaker_encoder / set_speakers)'
    dev = mel.device
    index = {s: i for i, s in enumerate(encoder.speaker_ids)}
    ids = target_ids.tolist() if torch.is_tensor(target_ids) else list(target_ids)
    target = torch.tensor([index.get(int(s), -1) for s in ids], dtype=torch.int64, device=dev)
    with torch.no_grad():
        n_frames = n_frames.long()
        emb = encoder.embed(mel, n_frames)
        cos = emb @ encoder.centroids.to(dev).t()                                        # (B, S)
        ok = (target >= 0) & (n_frames > 0)
        mine = F.one_hot(target.clamp(min=0), cos.shape[1]).bool()
        nan = torch.full((), float('nan'), dtype=torch.float32, device=dev)
        cos_target = torch.where(ok, cos[mine], nan)
        others = cos.masked_fill(mine, float('-inf')).max(dim=1).values
        scores = {'cos_target': cos_target, 'margin': torch.where(ok, cos_target - others, nan),
                  'identified': ok & (cos.argmax(dim=1) == target),
                  'accepted': ok & (cos_target >= encoder.threshold) if encoder.threshold is not None else torch.zeros_like(ok)}
        if reference_embeddings is not None:
            scores[REFERENCE_KEY] = torch.where(n_frames > 0, (emb * reference_embeddings.to(dev)).sum(dim=1), nan)
    return scores


def audio_speaker_scores(encoder, wavs, n_samples, target_ids, hparams, reference_embeddings=None):
    ''' `speaker_scores` of waveforms: wavs (B, S) fp32 / n_samples (B,) int64 on the device are analysed with
        `mel_spectrogram_batch`.  The front end's reflect padding needs more than half a window of samples: a shorter row (an empty
        synthesis) is not analysed, keeps 0 frames and scores NaN / not identified. '''
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
    return speaker_scores(encoder, mel, n_frames, target_ids, reference_embeddings)


def scores_to_host(scores):
    ''' {key: list} of `speaker_scores`' result, for a report '''
    return {key: value.cpu().tolist() for key, value in scores.items()}


def nearest_speakers(encoder, embeddings):
    ''' the speaker id whose centroid is nearest to every unit embedding (B, dim): a list '''
    nearest = (embeddings @ encoder.centroids.to(embeddings.device).t()).argmax(dim=1).cpu().tolist()
    return [encoder.speaker_ids[i] for i in nearest]


# ---- training and checkpoints ----------------------------------------------------------------------------------------------------------

def save_speaker_encoder(encoder, path):
    ''' the constructor arguments, the weights, the speaker ids with their centroids, the threshold and the EER '''
    torch.save({'args': dict(encoder.args), 'state_dict': {k: v.detach().cpu() for k, v in encoder.state_dict().items()},
                'speaker_ids': list(encoder.speaker_ids), 'centroids': encoder.centroids.detach().cpu(), 'threshold': encoder.threshold,
                'eer': encoder.eer}, path)


def load_speaker_encoder(path, device='cuda:0'):
    chk = torch.load(path, map_location='cpu')
    encoder = SpeakerEncoder(**chk['args'])
    encoder.load_state_dict(chk['state_dict'])
    encoder = encoder.to(H.device(device)).eval()
    encoder.set_speakers(chk['speaker_ids'], chk['centroids'], chk['threshold'], chk['eer'])
    return encoder


def list_speakers(list_file):
    ''' the speaker id of every line of a `features_dir|feature_file|speaker_id` list '''
    with open(list_file, 'r', encoding='utf-8') as f:
        return [int(line.strip().split('|')[2]) for line in f if line.strip()]


def read_items(list_file, hparams, device, batch_size=64):
    ''' [(speaker id, mel (n_mel, T) fp32, name)] on the device, in the list's order: `recognizer.read_items` with the speaker id
        (`batch[10]` of the collate) in place of the symbols '''
    from daft_exprt.data_loader import DaftExprtDataCollate, DaftExprtDataLoader
    dataset, collate = DaftExprtDataLoader(list_file, hparams, shuffle=False), DaftExprtDataCollate(hparams)
    items = {}
    for start in range(0, len(dataset), int(batch_size)):
        batch = collate([dataset[i] for i in range(start, min(len(dataset), start + int(batch_size)))])
        mel = batch[8].to(device)
        for row, (n_frm, spk, feature_dir, feature_file) in enumerate(zip(batch[9].tolist(), batch[10].tolist(), batch[11], batch[12])):
            items[(feature_dir, feature_file)] = (int(spk), mel[row, :, :n_frm].float().clone(), feature_file)
    return [items[(line[0], line[1])] for line in dataset.data]          # (the collate sorts a batch by length)


def collate_items(items, device):
    ''' [(speaker id, mel, ...)] -> mel (B, n_mel, T) fp32 zero-padded, n_frames (B,) int64 '''
    B, T = len(items), max(1, max(i[1].shape[1] for i in items))
    mel = torch.zeros((B, items[0][1].shape[0], T), dtype=torch.float32, device=device)
    for b, item in enumerate(items):
        mel[b, :, :item[1].shape[1]] = item[1]
    return mel, torch.tensor([i[1].shape[1] for i in items], dtype=torch.int64, device=device)


def embed_items(encoder, items, device, batch_size=64):
    ''' the unit embeddings (len(items), dim) of a list of items, batch_size at a time, without gradients '''
    out = []
    with torch.no_grad():
        for start in range(0, len(items), int(batch_size)):
            out.append(encoder.embed(*collate_items(items[start: start + int(batch_size)], device)))
    return torch.cat(out) if out else torch.zeros((0, encoder.args['dim']), device=device)


def speaker_centroids(embeddings, classes, n_speakers):
    ''' one row per speaker: the mean of the unit embeddings of its utterances, brought back to unit length '''
    sums = torch.zeros((n_speakers, embeddings.shape[1]), dtype=embeddings.dtype, device=embeddings.device).index_add_(0, classes, embeddings)
    return F.normalize(sums / torch.bincount(classes, minlength=n_speakers).clamp(min=1)[:, None].to(embeddings.dtype), dim=1)


def held_out_report(encoder, embeddings, classes):
    ''' of held-out unit embeddings (N, dim) with their speaker classes (N,) int64 against `encoder.centroids`: identification_error
        (the share whose nearest centroid is not their speaker), eer and threshold over ALL pairs (`trial_counts`,
        `eer_from_counts`; None when a class of trials is empty), trials (targets, non-targets), per_speaker {id: count, errors} '''
    nearest = (embeddings @ encoder.centroids.to(embeddings.device).t()).argmax(dim=1)
    wrong = (nearest != classes)
    counts = trial_counts(embeddings.contiguous(), classes.to(torch.int32))
    rates = eer_from_counts(counts)
    per_speaker = {}
    for c, speaker in enumerate(encoder.speaker_ids):
        mine = classes == c
        per_speaker[str(speaker)] = {'count': int(mine.sum()), 'errors': int((wrong & mine).sum())}
    return dict(identification_error=float(wrong.float().mean()), eer=None if rates is None else rates[0],
                threshold=None if rates is None else rates[1], trials=[int(counts[0].sum()), int(counts[1].sum())], per_speaker=per_speaker)


def train_speaker_encoder(hparams, training_files, validation_files, steps=2000, batch_size=32, lr=1e-3, seed=1234, hidden=256, layers=3,
                          stride=2, dim=128, scale=30.0, margin=0.2, log_every=100, device='cuda:0'):
    ''' trains a `SpeakerEncoder` on the utterances a `features_dir|feature_file|speaker_id` list names and returns (the model, a
        report).  Mels and speaker ids are read once through the data loader and its collate (`read_items`) and kept on the device;
        every step takes the next batch_size of a seeded permutation (one per epoch), Adam at `lr` on `am_softmax_loss` over the
        speakers of the training list -- fewer than 2 raise ValueError.  Utterances without a frame or with more steps
        (ceil(frames / stride)) than `attn_stat_pool` admits, and held-out utterances of a speaker the training list lacks, are left
        out and counted.  After training every speaker gets its centroid (`speaker_centroids` over the training utterances), and the
        held-out utterances give the report: utterances_train, utterances_held_out, speakers, steps, loss (the last step's),
        left_out, and -- None / empty without a held-out utterance -- identification_error, eer, threshold, trials, per_speaker of
        `held_out_report`.  The encoder returned carries the centroids, the threshold and the EER. '''
    speakers = sorted(set(list_speakers(training_files)))
    if len(speakers) < 2:
        raise ValueError(f'train_speaker_encoder: {len(speakers)} speaker in {training_files}: telling speakers apart takes at least 2')
    dev = H.device(device)
    class_of = {s: c for c, s in enumerate(speakers)}
    max_t = limits()[1] * int(stride)
    read = read_items(training_files, hparams, dev)
    items = [i for i in read if 0 < i[1].shape[1] <= max_t]
    read_held = read_items(validation_files, hparams, dev) if validation_files else []
    held = [i for i in read_held if 0 < i[1].shape[1] <= max_t and i[0] in class_of]
    left_out = len(read) - len(items) + len(read_held) - len(held)
    if not items:
        raise ValueError('train_speaker_encoder: no utterance to train on')
    _logger.info(f'train_speaker_encoder: {len(items)} utterances of {len(speakers)} speakers on the device, {len(held)} held out, '
                 f'{left_out} left out')
    torch.manual_seed(int(seed))
    encoder = SpeakerEncoder(int(hparams.n_mel_channels), hidden, layers, stride, dim).to(dev)
    class_weights = nn.Parameter(torch.randn((len(speakers), int(dim)), device=dev))
    classes = torch.tensor([class_of[i[0]] for i in items], dtype=torch.int64, device=dev)
    encoder.train()
    optimizer = torch.optim.Adam(list(encoder.parameters()) + [class_weights], lr=float(lr))
    gen = torch.Generator().manual_seed(int(seed))
    loss, order = None, []
    for step in range(int(steps)):
        if len(order) < min(int(batch_size), len(items)):
            order = torch.randperm(len(items), generator=gen).tolist()
        idx, order = order[:int(batch_size)], order[int(batch_size):]
        mel, n_frm = collate_items([items[i] for i in idx], dev)
        loss = am_softmax_loss(encoder(mel, n_frm), class_weights, classes[torch.tensor(idx, device=dev)], scale, margin)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        if log_every and (step % int(log_every) == 0 or step == int(steps) - 1):
            _logger.info(f'train_speaker_encoder: step {step} -- additive-margin softmax loss {float(loss.detach()):.5f}')
    encoder.eval()
    encoder.set_speakers(speakers, speaker_centroids(embed_items(encoder, items, dev), classes, len(speakers)))
    report = dict(utterances_train=len(items), utterances_held_out=len(held), speakers=len(speakers), steps=int(steps),
                  loss=float(loss.detach()) if loss is not None else None, identification_error=None, eer=None, threshold=None,
                  trials=[0, 0], per_speaker={}, left_out=left_out)
    if held:
        held_classes = torch.tensor([class_of[i[0]] for i in held], dtype=torch.int64, device=dev)
        report.update(held_out_report(encoder, embed_items(encoder, held, dev), held_classes))
        encoder.threshold, encoder.eer = report['threshold'], report['eer']
    return encoder, report
