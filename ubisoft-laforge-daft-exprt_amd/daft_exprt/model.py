"""DaftExprt acoustic model on hand-written gfx950 kernels.

Keeps the reference's Python surface (`src/daft_exprt/model.py:713-923`): `DaftExprt(hparams)`,
`parse_batch`, `forward(inputs)` (5-tuple, `model.py:780-787`), `inference(inputs, pitch_transform,
hparams)`, `get_int_durations`, `pitch_shift`, `pitch_multiply`, and the exact `state_dict` key set /
shapes (checkpoint ABI) -- but none of its arithmetic runs through ATen: every tensor op of
the hot path is an entry point of `libdaftexprt_hip.so` (include/daft_exprt_hip.h).

MI355X-first structure
  * parameters live in ONE flat fp32 buffer (views are exposed under the reference names); gradients
    in a second flat buffer -> Adam is one kernel over 14.7 M floats and the data-parallel all-reduce
    is a handful of large contiguous RCCL calls;
  * the backward pass is written out by hand (no autograd graph, no per-op Python dispatch beyond the
    kernel launches): `forward` records the few activations each kernel needs, `_backward` walks them
    in reverse.  A single `torch.autograd.Function` node bridges to `loss.backward()` for drop-in use;
  * MFMA operands are bf16 (or exact fp32 with `hparams.compute_dtype='fp32'`); the residual stream,
    LayerNorm statistics, softmax, Gaussian upsampling, the small heads, losses and Adam are fp32;
  * positional encodings, masks, the integer duration conversion and the prosody controls run on the
    device -- the reference's per-utterance host loops (`model.py:142-148, 799-808, 822-832, 849-862`)
    are gone.
There is no CPU fallback: CPU tensors raise.
"""
import math

import numpy as np
import torch
from torch import nn

from daft_exprt import config, ops, streams

_MASK63 = (1 << 63) - 1


def get_mask_from_lengths(lengths):
    ''' (B,) -> (B, max(lengths)) bool, True = valid (`model.py:14-24`).  Kept for API parity; the kernels
        take `lengths` directly and never materialise masks. '''
    ids = torch.arange(0, int(lengths.max()), device=lengths.device)
    return ids < lengths.unsqueeze(1)


# ------------------------------------------------------------------------------------------------
# parameter table: names / shapes / init families in the reference's registration order
# ------------------------------------------------------------------------------------------------
def film_layout(hp):
    ''' (nb_blocks, channels) per FiLM-ed module, projection-column order (`model.py:322-326`) '''
    return [(hp.phoneme_encoder['nb_blocks'], hp.phoneme_encoder['hidden_embed_dim']),
            (hp.local_prosody_predictor['nb_blocks'], hp.local_prosody_predictor['conv_channels']),
            (hp.frame_decoder['nb_blocks'], hp.phoneme_encoder['hidden_embed_dim'])]


def param_table(hp):
    ''' [(name, shape, init)], init in {'xavier:<gain>', 'ones', 'zeros', 'bias:<fan_in>', 'kaiming:<fan_in>'} '''
    T = []
    relu, lin = math.sqrt(2.), 1.
    n_mel, D = hp.n_mel_channels, hp.prosody_encoder['hidden_embed_dim']
    E = hp.phoneme_encoder['hidden_embed_dim']

    def conv(name, cout, cin, k, gain):
        T.append((f'{name}.conv.weight', (cout, cin, k), f'xavier:{gain}'))
        T.append((f'{name}.conv.bias', (cout,), f'bias:{cin * k}'))

    def linear(name, out, inp, gain):
        T.append((f'{name}.linear_layer.weight', (out, inp), f'xavier:{gain}'))
        T.append((f'{name}.linear_layer.bias', (out,), f'bias:{inp}'))

    def layer_norm(name, c):
        T.append((f'{name}.weight', (c,), 'ones'))
        T.append((f'{name}.bias', (c,), 'zeros'))

    def fft_blocks(pre, cfg, dim):
        for b in range(cfg['nb_blocks']):
            a = f'{pre}.blocks.{b}.attention'
            T.append((f'{a}.multi_head_attention.in_proj_weight', (3 * dim, dim), 'xavier:1.0'))
            T.append((f'{a}.multi_head_attention.in_proj_bias', (3 * dim,), 'zeros'))
            T.append((f'{a}.multi_head_attention.out_proj.weight', (dim, dim), f'kaiming:{dim}'))
            T.append((f'{a}.multi_head_attention.out_proj.bias', (dim,), 'zeros'))
            layer_norm(f'{a}.layer_norm', dim)
            f = f'{pre}.blocks.{b}.feed_forward'
            conv(f'{f}.convs.0', cfg['conv_channels'], dim, cfg['conv_kernel'], relu)
            conv(f'{f}.convs.2', dim, cfg['conv_channels'], cfg['conv_kernel'], lin)
            layer_norm(f'{f}.layer_norm', dim)

    cfg = hp.prosody_encoder
    C, K = cfg['conv_channels'], cfg['conv_kernel']
    if hp.post_mult_weight != 0.:
        T.append(('prosody_encoder.post_multipliers', (2, sum(nb for nb, _ in film_layout(hp))), 'xavier:1.0'))
    conv('prosody_encoder.energy_embedding', D, 1, K, lin)
    conv('prosody_encoder.pitch_embedding', D, 1, K, lin)
    for idx, (cin, cout) in zip((0, 4, 8), ((n_mel, C), (C, C), (C, D))):
        conv(f'prosody_encoder.convs.{idx}', cout, cin, K, relu)
        layer_norm(f'prosody_encoder.convs.{idx + 2}', cout)
    fft_blocks('prosody_encoder', cfg, D)
    T.append(('prosody_encoder.spk_embedding.weight', (hp.n_speakers, D), 'xavier:1.0'))
    nb_film = sum(nb * ch for nb, ch in film_layout(hp))
    linear('prosody_encoder.gammas_predictor', nb_film, D, lin)
    linear('prosody_encoder.betas_predictor', nb_film, D, lin)
    for idx, (i, o, gain) in zip((1, 3, 5), ((D, D, relu), (D, D, relu), (D, hp.n_speakers - 1, lin))):
        linear(f'speaker_classifier.classifier.{idx}', o, i, gain)
    T.append(('phoneme_encoder.symbols_embedding.weight', (hp.n_symbols, E), 'xavier:1.0'))
    fft_blocks('phoneme_encoder', hp.phoneme_encoder, E)
    cfg = hp.local_prosody_predictor
    for b in range(cfg['nb_blocks']):
        cin = E if b == 0 else cfg['conv_channels']
        for idx, ci in ((0, cin), (4, cfg['conv_channels'])):
            conv(f'prosody_predictor.blocks.{b}.{idx}', cfg['conv_channels'], ci, cfg['conv_kernel'], relu)
            layer_norm(f'prosody_predictor.blocks.{b}.{idx + 2}', cfg['conv_channels'])
    linear('prosody_predictor.projection', 3, cfg['conv_channels'], lin)
    Kg = hp.gaussian_upsampling_module['conv_kernel']
    for nm in ('duration_projection', 'energy_projection', 'pitch_projection'):
        conv(f'gaussian_upsampling.{nm}', E, 1, Kg, lin)
    T.append(('gaussian_upsampling.projection.0.linear_layer.weight', (1, E), f'xavier:{relu}'))
    T.append(('gaussian_upsampling.projection.0.linear_layer.bias', (1,), f'bias:{E}'))
    fft_blocks('frame_decoder', hp.frame_decoder, E)
    linear('frame_decoder.projection', n_mel, E, lin)
    return T


def _init_tensor(shape, init, gen):
    kind, _, arg = init.partition(':')
    if kind == 'ones':
        return torch.ones(shape)
    if kind == 'zeros':
        return torch.zeros(shape)
    u = torch.rand(shape, generator=gen) * 2 - 1
    if kind == 'xavier':   # nn.init.xavier_uniform_ (model.py:64, 84, 371, 387, 482)
        rf = int(np.prod(shape[2:])) if len(shape) > 2 else 1
        return u * (float(arg) * math.sqrt(6. / ((shape[0] + shape[1]) * rf)))
    return u / math.sqrt(float(arg))   # torch default Linear / Conv1d bias and kaiming(a=sqrt 5) weight bound


class _Node(nn.Module):
    ''' name-only container: reproduces the reference's module tree so that state_dict keys match '''


class _Saved(object):
    ''' bag of activations kept by the forward pass for the hand-written backward pass '''


class _Geometry(object):
    ''' what the kernels of one pass need to know about one lengths tensor (B, N rows), built once per pass and handed down to
        every stage that reads it (their saved records keep it for the backward pass):
          skip, nmax  the `skip_lengths` argument and the per-utterance hard sequence end: inside a grouped step
                      (`data_loader.GroupedBatch.bounds`) min(length, n_max - 2) of the utterance's own micro-batch and n_max (rows
                      at or past it are written as zeros); else the lengths themselves and None
          plan        balanced position tiles for the LayerNorm-fused k = 3 GEMMs (`ops.conv_tile_plan`), bf16 with
                      `balanced_tiles` only (else None)
          order       longest-first launch order of the attention kernels (`ops.length_order`), B >= 2 only (else None)
          wide        balanced tiles for the wide pre-net / predictor GEMMs (`dx_conv1d_wide`, halo 2, tile count a multiple of 64),
                      bf16 only (else None)
        plan, order and -- outside a grouped step -- wide come from ONE launch (`ops.batch_prep`).  In a grouped step wide is built
        from skip on first use, on the stream current then. '''

    def __init__(self, model, lengths, N, bounds=None):
        self.lengths, self.N = lengths, N
        self.skip, self.nmax = (lengths, None) if bounds is None else bounds
        self._bf = model.cd == torch.bfloat16
        plan, wide, order = self._bf and model.balanced_tiles, self._bf and bounds is None, lengths.shape[0] >= 2
        self.plan = self._wide = self.order = None
        if lengths.is_cuda and (self._bf or order):
            self.plan, self._wide, self.order = ops.batch_prep(lengths, N, plan, wide, order)

    @property
    def wide(self):
        if self._wide is None and self._bf:
            self._wide = ops.conv_tile_plan(self.skip, self.N, halo=2, round_to=64)
        return self._wide


# the events of the work the training step hands to the weight-gradient stream (see `DaftExprt.overlap_predictor`): the forks, in
# pass order, and the points the launch stream joins back at ('... done')
_HANDOFFS = ('classifier fwd', 'predictor fwd', 'predictor fwd done', 'predictor bwd', 'predictor bwd done', 'classifier bwd done',
             'upsampler grads', 'embedding grad')


class _Beside(object):
    ''' `with _Beside(side, events, name) as fork:` runs the body on stream `side` behind everything the current stream has issued
        so far (events[name] recorded there, waited for on `side`), or in line when `side` is None.  `fork.mark(done)` records
        events[done] on `side`, where the launch stream joins later.  A plain class rather than a generator-based context manager:
        it sits in the host-bound phoneme-level stretches of the step. '''
    __slots__ = ('side', 'events', 'name', 'ctx')

    def __init__(self, side, events, name):
        self.side, self.events, self.name = side, events, name

    def __enter__(self):
        if self.side is not None:
            ev = self.events[self.name]
            ev.record()
            self.side.wait_event(ev)
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def mark(self, done):
        if self.side is not None:
            self.events[done].record(self.side)

    def __exit__(self, *exc):
        if self.side is not None:
            self.ctx.__exit__(*exc)


class _Bridge(torch.autograd.Function):
    ''' one autograd node for the whole model: lets `loss.backward()` (reference train loop, train.py:391)
        drive the hand-written backward pass; parameter gradients are written into the flat buffer. '''
    @staticmethod
    def forward(ctx, anchor, model, saved, *outs):
        ctx.model, ctx.saved = model, saved
        return tuple(o.view_as(o) for o in outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._backward(ctx.saved, *grads)
        return (None, None, None) + (None,) * len(grads)


class DaftExprt(nn.Module):
    def __init__(self, hparams):
        super(DaftExprt, self).__init__()
        hparams.frame_decoder['hidden_embed_dim'] = hparams.phoneme_encoder['hidden_embed_dim']  # model.py:675
        self.hp = hparams
        # the kernels are specialised for the published architecture family: reject anything else up front instead of
        # failing inside an op (the reference would build any width; the checkpoint ABI of SURVEY 8b is the 128-wide one)
        dims = (hparams.prosody_encoder['hidden_embed_dim'], hparams.phoneme_encoder['hidden_embed_dim'])
        if dims != (128, 128):
            raise NotImplementedError(f'hidden_embed_dim of prosody_encoder / phoneme_encoder must be 128 / 128 (got {dims}): '
                                      'the residual-stream kernels (LayerNorm-fused GEMM epilogues, positional gather, '
                                      'attention head split) are built for 128 channels')
        for cfg, nm in ((hparams.prosody_encoder, 'prosody_encoder'), (hparams.phoneme_encoder, 'phoneme_encoder'),
                        (hparams.frame_decoder, 'frame_decoder')):
            # head sizes 16 and 64 (the published 8 / 2 heads) are the tuned attention kernels; 32 and 128 (4 heads / 1 head) run on
            # the same templates untuned (two-pass backward; the 128-wide head keeps one wave per SIMD)
            # conv_kernel 1 (the FF blocks as two linear layers, the prosody encoder's pre-net and scalar embeddings with one tap) runs on
            # the k = 1 GEMM kernels -- generic tiles, LayerNorm-fused epilogues, k = 1 weight gradients -- untuned: the register-weights
            # / split-K / wide kernels are k = 3 only.  5 taps have no kernel (the dead-row contract of DESIGN 2 is derived for a halo of
            # one row per conv)
            if 128 % cfg['attn_nb_heads'] or 128 // cfg['attn_nb_heads'] not in (16, 32, 64, 128) or cfg['conv_kernel'] not in (1, 3):
                raise NotImplementedError(f'{nm}: attention kernels exist for attn_nb_heads 8, 4, 2, 1 (head sizes 16 .. 128) and conv '
                                          f'kernels for conv_kernel 1 / 3, got attn_nb_heads={cfg["attn_nb_heads"]}, conv_kernel={cfg["conv_kernel"]}')
        if hparams.local_prosody_predictor['conv_kernel'] not in (1, 3):
            raise NotImplementedError(f'local_prosody_predictor: conv kernels exist for conv_kernel 1 / 3, got {hparams.local_prosody_predictor["conv_kernel"]}')
        if hparams.gaussian_upsampling_module['conv_kernel'] != 3:      # the upsampler's projection kernels (`dx_gu_prepare`, its backward) are three-tap
            raise NotImplementedError(f'gaussian_upsampling_module: conv_kernel must be 3, got {hparams.gaussian_upsampling_module["conv_kernel"]}')
        self.cd = torch.bfloat16 if getattr(hparams, 'compute_dtype', 'bf16') == 'bf16' else torch.float32
        self._table = param_table(hparams)
        gen = torch.Generator().manual_seed(int(torch.initial_seed()) & 0x7fffffff)
        for name, shape, init in self._table:
            node, parts = self, name.split('.')
            for part in parts[:-1]:
                if not hasattr(node, part):
                    node.add_module(part, _Node())
                node = getattr(node, part)
            node.register_parameter(parts[-1], nn.Parameter(_init_tensor(shape, init, gen)))
        assert [n for n, _ in self.named_parameters()] == [n for n, _, _ in self._table]
        self._flat = self._gflat = None
        self._packed, self._packed_version, self._param_version = {}, -1, 0
        self._adam_table = {}
        # True (default, always safe): re-pack the bf16 weight copies on every call (one batched kernel, ~40 us).  False: re-pack only
        # when the parameters changed through torch -- `_weights` watches the version counters of the GEMM weights, so
        # load_state_dict, torch.optim steps and in-place ops under no_grad are all seen; writes through `.data`, `model._P[...]`
        # or the flat buffer are NOT (EMA swaps, weight clipping): those callers use `mark_updated()`.  `Trainer`, which owns every
        # parameter update, switches it off.
        self.always_repack = True
        self._anchor = None
        self._side = self._side_stream = None
        self._wgrad_keep = []
        self._wgrad_pending = []
        self._wgrad_ws = None
        self._hop = None
        self._side_deferred = None
        self.fuse_ln_backward = True   # see _fft_block_bwd (tests compare against the separate LayerNorm-backward launches)
        self.balanced_tiles = True     # see _Geometry.plan (tests compare against the fixed-tile launches)
        self._geometry = ()            # the _Geometry records of the latest pass: their plan buffers live until the next pass starts
        # the local prosody predictor beside the decoder: in a teacher-forced step its forward feeds nothing but the loss and its backward
        # needs nothing but the loss gradients, so both run on the weight-gradient stream (idle in the forward pass, a FIFO of launches
        # that nobody waits for in the backward pass) while the launch stream goes on with upsampling and decoder.  The same holds for
        # the speaker classifier (forward and backward) and for the launches of the backward pass that only produce parameter gradients
        # (Gaussian upsampling's three, the symbol embedding's): ~45 launches of 5-30 us off the critical path, 6.51 -> 6.34 ms per
        # step.  False: everything in line, as before (tests compare the two)
        self.overlap_predictor = True
        self._handoff = None
        self._step_id, self._site, self._rank, self._capture_step0 = 0, 0, 0, 0
        self._seed_log = None
        self._trace = None    # tests set this to a list: every stage appends (kind, names, input, film, lengths, output)
        self._trace_bwd = None   # likewise for the backward pass: (kind, saved, saved_below, gradient in, gradient out)
        self._pos = None
        self.n_params = sum(int(np.prod(s)) for _, s, _ in self._table)
        self._gemm_weights = [n for n, s, _ in self._table if
                              (n.endswith('conv.weight') and s[1] > 1) or n.endswith('in_proj_weight') or
                              n.endswith('out_proj.weight') or n == 'frame_decoder.projection.linear_layer.weight']
        self._flatten()

    # ------------------------------------------------------------------ flat parameter / gradient storage
    def _apply(self, fn, *args, **kwargs):
        out = super(DaftExprt, self)._apply(fn, *args, **kwargs)
        self._flatten()
        return out

    def _flatten(self):
        params = self._params = dict(self.named_parameters())
        dev = next(iter(params.values())).device
        flat = torch.empty(self.n_params, dtype=torch.float32, device=dev)
        gflat = torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        off = 0
        self._P, self._G, self._offsets = {}, {}, {}
        for name, shape, _ in self._table:
            n = int(np.prod(shape))
            p = params[name]
            flat[off: off + n].copy_(p.data.reshape(-1).float())
            p.data = flat[off: off + n].view(shape)
            p.grad = gflat[off: off + n].view(shape)
            self._P[name], self._G[name], self._offsets[name] = p.data, p.grad, (off, n)
            off += n
        self._flat, self._gflat = flat, gflat
        self._pos = None
        self._packed = {}
        self._adam_table = {}
        self.mark_updated()

    def flat_parameters(self):
        return self._flat

    def flat_gradients(self):
        return self._gflat

    def mark_updated(self):
        ''' call after the parameters changed outside of this module (optimizer step) '''
        self._param_version += 1

    def zero_grad(self, set_to_none=False):
        if self._gflat is None:
            return super(DaftExprt, self).zero_grad(set_to_none)
        if self._gflat.is_cuda:
            ops.H.check(ops.H.lib().dx_fill_zero(ops.H.ptr(self._gflat), self._gflat.numel() * 4, ops.H.stream()))
        else:
            self._gflat.zero_()
        for name, p in self._params.items():   # an external optimizer may have dropped the views
            if p.grad is None or p.grad.data_ptr() != self._G[name].data_ptr():
                p.grad = self._G[name]

    def load_state_dict(self, state_dict, strict=True):
        out = super(DaftExprt, self).load_state_dict(state_dict, strict)
        self.mark_updated()
        return out

    # ------------------------------------------------------------------ device-side constants
    def _pos_table(self):
        ''' sinusoid table of `PositionalEncoding.__init__` (`model.py:123-130`), built with the same torch
            ops so that it is bit-identical, uploaded once. '''
        if self._pos is None:
            dim, max_len = self.hp.phoneme_encoder['hidden_embed_dim'], 5000
            pos = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
            div = torch.exp(torch.arange(0, dim, 2).float() * (-np.log(10000.) / dim))
            table = torch.zeros(max_len, dim)
            table[:, 0::2] = torch.sin(pos * div)
            table[:, 1::2] = torch.cos(pos * div)
            self._pos = table.to(self._flat.device)
        return self._pos

    def _weights(self, need_dgrad):
        ''' MFMA-operand copies of the GEMM weights (compute dtype): forward packing [tap][Cout][Cin] and
            data-gradient packing [tap][Cin][Cout] with flipped taps, refreshed by batched kernel launches (the training step never
            gets here: its optimizer launch refreshes every copy, `packs_are_current`). '''
        if not self._packed:
            dev, fwd, bwd = self._flat.device, ([], []), []
            early = lambda name: name.startswith('prosody_encoder.convs.')
            for name in self._gemm_weights:
                w = self._P[name]
                taps = w.shape[2] if w.dim() == 3 else 1
                self._packed[name] = torch.empty((taps, w.shape[0], w.shape[1]), dtype=self.cd, device=dev)
                fwd[0 if early(name) else 1].append((w, self._packed[name], False))
                if name != 'prosody_encoder.convs.0.conv.weight':   # the mel input needs no gradient
                    self._packed['T:' + name] = torch.empty((taps, w.shape[1], w.shape[0]), dtype=self.cd, device=dev)
                    bwd.append((w, self._packed['T:' + name], True))
            self._pack_fwd = [ops.pack_table(f, dev) if f else None for f in fwd]   # [pre-net, everything else]
            self._pack_bwd = ops.pack_table(bwd, dev)
            # fragment-order copies ('F:' of the forward matrix, 'FT:' of the data-gradient matrix) of the k = 3 weights, one contiguous KiB
            # per MFMA fragment: a matrix gets one exactly when a kernel that reads fragments from L2 straight into registers takes its
            # (Cin, Cout) -- the wide kernel, the register-weights kernel or the split-K workgroups (the predicates of ops)
            self._frag_fwd, self._frag_bwd = [None, None], None
            if self.cd == torch.bfloat16:
                ffwd, fbwd = ([], []), []
                for name in self._gemm_weights:
                    w = self._P[name]
                    if w.dim() != 3 or w.shape[2] != 3:
                        continue
                    # The wide kernel goes by shape alone.  The other two are handed a copy by the FF blocks only: a pre-net or predictor conv
                    # of a matching shape (128 -> 256, k = 3) passes W.get('F:...') to ops.conv1d, which would hand the copy to
                    # dx_conv1d_wfrag -- another load path for that GEMM
                    is_ff = '.feed_forward.convs.' in name
                    reads = lambda cin, cout: ops.wide_shape_ok(cin, cout) or (
                        is_ff and (ops.wreg_shape_ok(cin, cout) or ops.splitk_shape_ok(cin, cout)))
                    cout, cin = w.shape[0], w.shape[1]
                    if reads(cin, cout):
                        self._packed['F:' + name] = torch.empty(w.numel(), dtype=self.cd, device=dev)
                        ffwd[0 if early(name) else 1].append((self._packed[name], self._packed['F:' + name]))
                    if 'T:' + name in self._packed and reads(cout, cin):
                        self._packed['FT:' + name] = torch.empty(w.numel(), dtype=self.cd, device=dev)
                        fbwd.append((self._packed['T:' + name], self._packed['FT:' + name]))
                self._frag_fwd = [ops.frag_table(f, dev) if f else None for f in ffwd]
                self._frag_bwd = ops.frag_table(fbwd, dev) if fbwd else None
            self._packed_version = self._dgrad_version = -1
        try:
            version = (self._param_version, tuple(self._params[n]._version for n in self._gemm_weights))
        except RuntimeError:      # inference tensors (model built or moved under torch.inference_mode()) carry no version counter
            version = (self._param_version, None)
            self._packed_version = -1 if self._packed_version == version else self._packed_version   # always re-pack
        do_fwd = self._packed_version != version or self.always_repack
        do_bwd = need_dgrad and (do_fwd or self._dgrad_version != self._packed_version)
        if not (do_fwd or do_bwd):
            return self._packed
        if do_fwd:
            for tab in self._pack_fwd:
                if tab is not None:
                    ops.pack_weights_batched(*tab, self.cd)
            for tab in self._frag_fwd:
                if tab is not None:
                    ops.pack_frag_major_batched(*tab)
            self._packed_version = version
            self._dgrad_version = -1
        if do_bwd:
            ops.pack_weights_batched(*self._pack_bwd, self.cd)
            if self._frag_bwd is not None:
                ops.pack_frag_major_batched(*self._frag_bwd)
            self._dgrad_version = self._packed_version
        return self._packed

    def adam_pack_table(self, rng=None):
        ''' the tables of `ops.adam_pack_step` (Adam fused with the refresh of the operand copies) for the copies `_weights` keeps, or
            None before the first forward pass has created them.  Every GEMM weight with its copies; every other parameter as
            flat ranges (merged where adjacent).  rng = (offset, numel): only the parameters inside that slice of the flat buffer
            (a gradient bucket of the data-parallel reducer; slices end on parameter boundaries). '''
        if not self._packed:
            return None
        if rng not in self._adam_table:
            W, gemm = self._packed, set(self._gemm_weights)
            weights, flats = [], []
            lo, hi = (0, self._flat.numel()) if rng is None else (rng[0], rng[0] + rng[1])
            for name, shape, _ in self._table:
                off, n = self._offsets[name]
                if off < lo or off >= hi:
                    continue
                assert off + n <= hi, f'{name} straddles the end of the slice'
                if name in gemm:
                    taps = shape[2] if len(shape) == 3 else 1
                    weights.append((off, (shape[0], shape[1], taps), W.get(name), W.get('T:' + name), W.get('F:' + name), W.get('FT:' + name)))
                elif flats and flats[-1][0] + flats[-1][1] == off:
                    flats[-1] = (flats[-1][0], flats[-1][1] + n)
                else:
                    flats.append((off, n))
            self._adam_table[rng] = ops.adam_pack_table(weights, flats, self._flat.device) if weights else None
        return self._adam_table[rng]

    def packs_are_current(self):
        ''' the optimizer has just refreshed EVERY operand copy together with the parameters (`ops.adam_pack_step`) '''
        try:
            version = (self._param_version, tuple(self._params[n]._version for n in self._gemm_weights))
        except RuntimeError:
            return
        self._packed_version = self._dgrad_version = version

    def set_rank(self, rank):
        ''' data-parallel rank of this replica: folded into every dropout seed so that the ranks draw independent masks
            (torch's per-process Philox streams in the reference are independent as well) '''
        self._rank = int(rank)

    def _seed(self, kind=None):
        ''' dropout seed of the next site of this forward pass: a function of (hparams seed, step, site, rank).  While a step is being
            captured (`ops.STEP_PTR` set) the absolute step stays out of the by-value seed -- only the micro-batch's offset from the
            capture's first one goes in -- and the kernels add `step_salt()` from the device-side step block: same sum mod 2^63, so
            a replayed step draws the masks the eager step with the same step id draws. '''
        self._site += 1
        step = self._step_id if ops.STEP_PTR is None else self._step_id - self._capture_step0
        seed = (int(self.hp.seed) * 0x9E3779B1 + step * 0x85EBCA77 + self._site * 0xC2B2AE3D +
                self._rank * 0x27D4EB2F165667C5) & _MASK63
        if self._seed_log is not None:      # tests/test_gpu_dropout_parity.py: the oracle draws the same masks from these
            self._seed_log.append((kind, seed))
        return seed

    def step_salt(self, step_id=None):
        ''' the step's share of every dropout seed, for the device-side step block (see `_seed`) '''
        return ((self._step_id if step_id is None else step_id) * 0x85EBCA77) & _MASK63

    # ------------------------------------------------------------------ reference surface
    def parse_batch(self, gpu, batch):
        ''' `model.py:727-753`: H2D (non-blocking) + dtype casts; same tuple orders '''
        dev = torch.device('cuda', gpu) if isinstance(gpu, int) else torch.device(gpu)
        symbols, durations_float, durations_int, symbols_energy, symbols_pitch, input_lengths, \
            frames_energy, frames_pitch, mel_specs, output_lengths, speaker_ids, feature_dirs, feature_files = batch
        self.check_ids(symbols, speaker_ids, training=True)
        f = lambda t: t.to(dev, non_blocking=True).float().contiguous()
        i = lambda t: t.to(dev, non_blocking=True).long().contiguous()
        inputs = (i(symbols), f(durations_float), i(durations_int), f(symbols_energy), f(symbols_pitch), i(input_lengths),
                  f(frames_energy), f(frames_pitch), f(mel_specs), i(output_lengths), i(speaker_ids))
        targets = (inputs[1], inputs[3], inputs[4], inputs[8], inputs[10])
        return inputs, targets, (feature_dirs, feature_files)

    def check_ids(self, symbols, speaker_ids, training):
        ''' index-range checks on HOST tensors (collate output), where they cost nothing: the reference raises in these
            cases (nn.Embedding / CrossEntropyLoss index errors), the gather kernels would read out of bounds silently.
            Device tensors are passed through unchecked (checking them would add a sync per batch). '''
        hp = self.hp
        if torch.is_tensor(symbols) and not symbols.is_cuda and symbols.numel():
            lo, hi = int(symbols.min()), int(symbols.max())
            if lo < 0 or hi >= hp.n_symbols:
                raise IndexError(f'symbol id out of range [0, {hp.n_symbols}): min {lo}, max {hi}')
        if torch.is_tensor(speaker_ids) and not speaker_ids.is_cuda and speaker_ids.numel():
            lo, hi = int(speaker_ids.min()), int(speaker_ids.max())
            top = hp.n_speakers - 1 if training else hp.n_speakers   # classifier targets (model.py:273) / embedding rows (366)
            if lo < 0 or hi >= top:
                raise IndexError(f'speaker id out of range [0, {top}): min {lo}, max {hi}')

    def forward(self, inputs):
        ''' `model.py:755-787` (teacher-forced).  Returns (speaker_preds, [post_multipliers, enc_film, pp_film,
            dec_film], [dur, energy, pitch, input_lengths], [mel (B, n_mel, T), output_lengths], weights). '''
        train = self.training
        need_grad = train and torch.is_grad_enabled()
        with torch.no_grad():
            outs, saved = self._forward(inputs, train, need_grad)
        spk, films, (dur, energy, pitch), mel, weights = outs
        input_lengths, output_lengths = inputs[5].detach(), inputs[9].detach()
        post = self._P['prosody_encoder.post_multipliers'] if self.hp.post_mult_weight != 0. else 1.
        if need_grad:
            if self._anchor is None or self._anchor.device != mel.device:
                self._anchor = torch.zeros(1, device=mel.device, requires_grad=True)
            post_param = self._params.get('prosody_encoder.post_multipliers')
            spk, dur, energy, pitch, mel = _Bridge.apply(self._anchor, self, saved, spk, dur, energy, pitch, mel)
            post = post_param if post_param is not None else 1.
        return spk, [post, films[0], films[1], films[2]], [dur, energy, pitch, input_lengths], \
            [mel, output_lengths], weights

    # ------------------------------------------------------------------ forward building blocks
    def _fft_block_fwd(self, W, pre, x, film, g, cfg, train, save, x_lp=None, qkv=None, next_pre=None):
        ''' one FFT block (`model.py:251-264`).  In bf16 mode the LayerNorm kernels also emit bf16 copies of their
            outputs (`*_lp`): they are what the following GEMMs read (half the bytes, no in-kernel conversion) --
            numerically identical to casting at operand-load time.  qkv: this block's QKV projection when the block below has
            already computed it (in the epilogue of its last launch); next_pre: the block above, whose QKV projection this block's
            last launch computes when it can.  Returns (u, u_lp, saved, qkv of the next block or None). '''
        P, cd = self._P, self.cd
        lp = cd == torch.bfloat16
        a_pre, f_pre = f'{pre}.attention', f'{pre}.feed_forward'
        p_attn = cfg['attn_dropout'] if train else 0.
        p_conv = cfg['conv_dropout'] if train else 0.
        s = _Saved() if save else None
        seeds = [self._seed(k) for k in ('attention weights', 'attention output', 'feed-forward output')]
        xin = x_lp if x_lp is not None else x
        if qkv is None:
            qkv = ops.conv1d(xin, W[f'{a_pre}.multi_head_attention.in_proj_weight'], P[f'{a_pre}.multi_head_attention.in_proj_bias'],
                             out_dtype=cd, skip_lengths=g.skip)
        o, lse = ops.attention_fwd(qkv, g.lengths, cfg['attn_nb_heads'], p_attn, seeds[0], need_lse=save, order=g.order)
        # out-projection + Dropout + residual + LayerNorm + mask in ONE launch (the GEMM tile holds complete 128-ch rows)
        # (training, bf16, split-K FF kernel: the fp32 copy of `a` has ONE reader, the residual add of the FF LayerNorm, which re-derives it
        #  from s1 and the row statistics -- ops.conv1d_ln `residual_ln`; `a` itself is then never stored)
        wc2, plan = W[f'{f_pre}.convs.2.conv.weight'], g.plan
        virt = bool(save and lp and config.VIRTUAL_RESIDUAL and self._trace is None and plan is not None and
                    ops.splitk_ln_ok(x.shape[0], x.shape[1], cd, wc2, plan, W.get(f'F:{f_pre}.convs.2.conv.weight')))
        a, a_lp, s1, mean1, rstd1 = ops.conv1d_ln(o, W[f'{a_pre}.multi_head_attention.out_proj.weight'],
                                                  P[f'{a_pre}.multi_head_attention.out_proj.bias'], x, P[f'{a_pre}.layer_norm.weight'],
                                                  P[f'{a_pre}.layer_norm.bias'], g.lengths, save=save, p_pre=p_attn, seed_pre=seeds[1],
                                                  lp_copy=lp, store_y=not virt)
        ain = a_lp if lp else a
        # (grouped step: the FF hidden is the one unmasked tensor whose row AT the sequence end reaches valid outputs -- mask it there)
        # (training, bf16: the ReLU also leaves one bit per element -- the gate of the data gradient reads those instead of h, ops.conv1d)
        hbits = None
        wc0 = W[f'{f_pre}.convs.0.conv.weight']
        if save and config.RELU_BITS and ops.relu_bits_ok(ain, wc0, cd):
            h, hbits = ops.conv1d(ain, wc0, P[f'{f_pre}.convs.0.conv.bias'], out_dtype=cd, relu=True, relu_bits=True,
                                  skip_lengths=g.skip, mask_lengths=g.nmax, w_frag=W.get(f'F:{f_pre}.convs.0.conv.weight'))
        else:
            h = ops.conv1d(ain, wc0, P[f'{f_pre}.convs.0.conv.bias'], out_dtype=cd, relu=True,
                           skip_lengths=g.skip, mask_lengths=g.nmax, w_frag=W.get(f'F:{f_pre}.convs.0.conv.weight'))
        # second FF conv + Dropout + residual + LayerNorm + FiLM + mask in ONE launch
        nmha = f'{next_pre}.attention.multi_head_attention' if (next_pre is not None and lp) else None
        u, u_lp, s2, mean2, rstd2, qkv_next = ops.conv1d_ln(
            h, wc2, P[f'{f_pre}.convs.2.conv.bias'], s1 if virt else a, P[f'{f_pre}.layer_norm.weight'], P[f'{f_pre}.layer_norm.bias'],
            g.lengths, film=film, save=save, p_pre=p_conv, seed_pre=seeds[2], lp_copy=lp, plan=plan,
            residual_ln=(mean1, rstd1, P[f'{a_pre}.layer_norm.weight'], P[f'{a_pre}.layer_norm.bias']) if virt else None,
            w_frag=W.get(f'F:{f_pre}.convs.2.conv.weight'), w2_packed=W[f'{nmha}.in_proj_weight'] if nmha else None,
            b2=P[f'{nmha}.in_proj_bias'] if nmha else None) + ((None,) if nmha is None else ())
        if save:
            s.pre, s.cfg, s.x, s.film, s.lengths, s.geo = pre, cfg, xin, film, g.lengths, g
            s.qkv, s.o, s.lse, s.s1, s.mean1, s.rstd1, s.a, s.h, s.s2, s.mean2, s.rstd2 = qkv, o, lse, s1, mean1, rstd1, ain, h, s2, mean2, rstd2
            s.seeds, s.p_attn, s.p_conv = seeds, p_attn, p_conv
            s.hbits = hbits
        if self._trace is not None:
            self._trace.append(('fft_block', pre, x, film, g.lengths, (a, u)))
        return u, u_lp, s, qkv_next

    def _conv_ln_fwd(self, W, conv_name, ln_name, x, p_drop, out_dtype, save, g, film=None, masked=False, wgrad_lengths=None):
        ''' conv k3 -> ReLU -> LayerNorm -> Dropout [-> FiLM -> mask]  (prenet `model.py:341-363`, predictor 528-566).  masked: rows past
            g.lengths are zeroed; wgrad_lengths: the lengths argument of the weight gradient in the backward pass '''
        P = self._P
        lengths, skip = g.lengths if masked else None, g.skip
        cout = P[f'{conv_name}.conv.weight'].shape[0]
        c_dtype = torch.float32 if (self.cd == torch.float32 or cout == 128) else self.cd   # wide tensors in the MFMA operand type
        c = ops.conv1d(x, W[f'{conv_name}.conv.weight'], P[f'{conv_name}.conv.bias'], relu=True, out_dtype=c_dtype, skip_lengths=skip,
                       w_frag=W.get(f'F:{conv_name}.conv.weight'), wide_plan=g.wide if f'F:{conv_name}.conv.weight' in W else None)
        seed = self._seed('behind LayerNorm')
        y, _, mean, rstd = ops.layernorm_fwd(c, P[f'{ln_name}.weight'], P[f'{ln_name}.bias'], film=film, lengths=lengths,
                                             out_dtype=out_dtype, save=save, p_post=p_drop, seed_post=seed, skip_lengths=skip)
        s = None
        if save:
            s = _Saved()
            s.conv_name, s.ln_name, s.x, s.c, s.mean, s.rstd, s.p, s.seed, s.film, s.lengths, s.skip = \
                conv_name, ln_name, x, c, mean, rstd, p_drop, seed, film, lengths, skip
            s.geo, s.wgrad_lengths = g, wgrad_lengths
        if self._trace is not None:
            self._trace.append(('conv_ln', (conv_name, ln_name, skip), x, film, lengths, y))
        return y, s

    def _prosody_encoder_fwd(self, W, frames_energy, frames_pitch, mel_specs, speaker_ids, g, train, save):
        ''' `model.py:391-464` '''
        P, hp, cfg, pre = self._P, self.hp, self.hp.prosody_encoder, 'prosody_encoder'
        p_conv = cfg['conv_dropout'] if train else 0.
        s = _Saved()
        # (B, T, n_mel) channel-last rows (no-op casts on the step path: parse_batch normalises); in bf16 mode the transpose emits bf16
        # = the rounding the first conv applies at operand load; its weight gradient (the last launch of the backward pass, nothing
        # left to hide it under) then runs on the LDS-DMA ring kernel
        x = ops.transpose_last2(mel_specs.float().contiguous(), torch.bfloat16 if self.cd == torch.bfloat16 else torch.float32)
        wide, output_lengths = self.cd, g.lengths
        l1, s.c1 = self._conv_ln_fwd(W, f'{pre}.convs.0', f'{pre}.convs.2', x, p_conv, wide, save, g, wgrad_lengths=output_lengths)
        l2, s.c2 = self._conv_ln_fwd(W, f'{pre}.convs.4', f'{pre}.convs.6', l1, p_conv, wide, save, g, wgrad_lengths=output_lengths)
        l3, s.c3 = self._conv_ln_fwd(W, f'{pre}.convs.8', f'{pre}.convs.10', l2, p_conv, torch.float32, save, g, wgrad_lengths=output_lengths)
        x0 = ops.scalar_embed_fwd([frames_energy, frames_pitch],
                                  [P[f'{pre}.energy_embedding.conv.weight'], P[f'{pre}.pitch_embedding.conv.weight']],
                                  [P[f'{pre}.energy_embedding.conv.bias'], P[f'{pre}.pitch_embedding.conv.bias']],
                                  base=l3, pos_table=self._pos_table(), lengths=output_lengths)
        s.blocks = []
        x_lp = qkv = None
        for blk in range(cfg['nb_blocks']):
            x0, x_lp, sb, qkv = self._fft_block_fwd(W, f'{pre}.blocks.{blk}', x0, None, g, cfg, train, save, x_lp, qkv,
                                                    f'{pre}.blocks.{blk + 1}' if blk + 1 < cfg['nb_blocks'] else None)
            s.blocks.append(sb)
        emb = ops.masked_mean_fwd(x0, output_lengths)
        layout = film_layout(hp)
        nb, ch = [n for n, _ in layout], [c for _, c in layout]
        post = P[f'{pre}.post_multipliers'] if hp.post_mult_weight != 0. else None
        if ops.USE_FUSED_HEADS:      # speaker-embedding add + both FiLM projections + the FiLM split in one launch
            z, g_raw, b_raw, films = ops.film_head_fwd(emb, P[f'{pre}.spk_embedding.weight'], speaker_ids,
                                                       P[f'{pre}.gammas_predictor.linear_layer.weight'], P[f'{pre}.gammas_predictor.linear_layer.bias'],
                                                       P[f'{pre}.betas_predictor.linear_layer.weight'], P[f'{pre}.betas_predictor.linear_layer.bias'],
                                                       post, nb, ch)
        else:
            z = ops.gather_add_fwd(emb, P[f'{pre}.spk_embedding.weight'], speaker_ids)
            g_raw = ops.linear_small_fwd(z, P[f'{pre}.gammas_predictor.linear_layer.weight'], P[f'{pre}.gammas_predictor.linear_layer.bias'])
            b_raw = ops.linear_small_fwd(z, P[f'{pre}.betas_predictor.linear_layer.weight'], P[f'{pre}.betas_predictor.linear_layer.bias'])
            films = ops.film_assemble_fwd(g_raw, b_raw, post, nb, ch)
        s.T, s.z, s.g_raw, s.b_raw, s.nb, s.ch, s.post = x0.shape[1], z, g_raw, b_raw, nb, ch, post
        s.frames_energy, s.frames_pitch, s.speaker_ids, s.output_lengths = frames_energy, frames_pitch, speaker_ids, output_lengths
        return emb, films, s

    def _fused_classifier(self):
        ''' the one-launch classifier holds its logits in a 128-wide tile: more than 129 speakers take the `linear_small_*` launches '''
        return ops.USE_FUSED_HEADS and self.hp.n_speakers - 1 <= 128

    def _classifier_fwd(self, emb):
        ''' `model.py:285-292`; the gradient reversal is an identity here and a sign flip in `_backward` '''
        P, pre = self._P, 'speaker_classifier.classifier'
        if self._fused_classifier():
            logits, h1, h2 = ops.classifier_fwd(emb, P[f'{pre}.1.linear_layer.weight'], P[f'{pre}.1.linear_layer.bias'], P[f'{pre}.3.linear_layer.weight'],
                                                P[f'{pre}.3.linear_layer.bias'], P[f'{pre}.5.linear_layer.weight'], P[f'{pre}.5.linear_layer.bias'])
            return logits, (emb, h1, h2)
        h1 = ops.linear_small_fwd(emb, P[f'{pre}.1.linear_layer.weight'], P[f'{pre}.1.linear_layer.bias'], relu=True)
        h2 = ops.linear_small_fwd(h1, P[f'{pre}.3.linear_layer.weight'], P[f'{pre}.3.linear_layer.bias'], relu=True)
        logits = ops.linear_small_fwd(h2, P[f'{pre}.5.linear_layer.weight'], P[f'{pre}.5.linear_layer.bias'])
        return logits, (emb, h1, h2)

    def _phoneme_encoder_fwd(self, W, symbols, film, g, train, save):
        ''' `model.py:490-509` '''
        cfg, pre = self.hp.phoneme_encoder, 'phoneme_encoder'
        x = ops.embed_pos_fwd(symbols, self._P[f'{pre}.symbols_embedding.weight'], self._pos_table(), g.lengths)
        blocks, x_lp, qkv = [], None, None
        for blk in range(cfg['nb_blocks']):
            x, x_lp, sb, qkv = self._fft_block_fwd(W, f'{pre}.blocks.{blk}', x, film[:, blk, :], g, cfg, train, save, x_lp, qkv,
                                                   f'{pre}.blocks.{blk + 1}' if blk + 1 < cfg['nb_blocks'] else None)
            blocks.append(sb)
        return x, blocks

    def _predictor_fwd(self, W, enc, film, g, train, save):
        ''' `model.py:549-575` (nb_blocks = 1 in every published config; more blocks chain the same pattern) '''
        cfg, pre, P = self.hp.local_prosody_predictor, 'prosody_predictor', self._P
        p = cfg['conv_dropout'] if train else 0.
        x, saved = enc, []
        for blk in range(cfg['nb_blocks']):
            x, s1 = self._conv_ln_fwd(W, f'{pre}.blocks.{blk}.0', f'{pre}.blocks.{blk}.2', x, p, self.cd, save, g)
            last = blk == cfg['nb_blocks'] - 1
            x, s2 = self._conv_ln_fwd(W, f'{pre}.blocks.{blk}.4', f'{pre}.blocks.{blk}.6', x, p, torch.float32 if last else self.cd,
                                      save, g, film=film[:, blk, :], masked=last)
            saved.append((s1, s2))
        L = x.shape[1]
        y = ops.linear_small_fwd(x, P[f'{pre}.projection.linear_layer.weight'], P[f'{pre}.projection.linear_layer.bias'],
                                 mask_lengths=g.lengths, N=L)
        return y, (saved, x, y)

    def _gu_params(self):
        P, pre = self._P, 'gaussian_upsampling'
        return {'w_dur': P[f'{pre}.duration_projection.conv.weight'], 'b_dur': P[f'{pre}.duration_projection.conv.bias'],
                'w_en': P[f'{pre}.energy_projection.conv.weight'], 'b_en': P[f'{pre}.energy_projection.conv.bias'],
                'w_pi': P[f'{pre}.pitch_projection.conv.weight'], 'b_pi': P[f'{pre}.pitch_projection.conv.bias'],
                'w_range': P[f'{pre}.projection.0.linear_layer.weight'], 'b_range': P[f'{pre}.projection.0.linear_layer.bias']}

    def _upsample_fwd(self, enc, durations_float, durations_int, energies, pitch, input_lengths, output_lengths, T, save):
        ''' `model.py:608-662` + the decoder's positional add and mask (`model.py:696-701`) '''
        GP = self._gu_params()
        xp, ranges, r_pre, rin = ops.gu_prepare(enc, durations_float, energies, pitch, input_lengths, GP, save=save)
        means, totals = ops.gu_means(durations_int)
        dec_in, weights = ops.gu_upsample_fwd(xp, ranges, means, input_lengths, T, output_lengths, self._pos_table())
        s = None
        if save:
            s = _Saved()
            s.xp, s.ranges, s.r_pre, s.rin, s.means, s.weights = xp, ranges, r_pre, rin, means, weights
            s.durations_float, s.energies, s.pitch, s.input_lengths, s.output_lengths = durations_float, energies, pitch, input_lengths, output_lengths
        return dec_in, weights, totals, s

    def _decoder_fwd(self, W, x, film, g, train, save):
        ''' `model.py:689-710` (positional add + mask already applied by the upsampling kernel) '''
        cfg, pre, P = self.hp.frame_decoder, 'frame_decoder', self._P
        blocks, x_lp, qkv = [], None, None
        for blk in range(cfg['nb_blocks']):
            x, x_lp, sb, qkv = self._fft_block_fwd(W, f'{pre}.blocks.{blk}', x, film[:, blk, :], g, cfg, train, save, x_lp, qkv,
                                                   f'{pre}.blocks.{blk + 1}' if blk + 1 < cfg['nb_blocks'] else None)
            blocks.append(sb)
        mel = ops.conv1d(x, W[f'{pre}.projection.linear_layer.weight'], P[f'{pre}.projection.linear_layer.bias'],
                         out_dtype=torch.float32, mask_lengths=g.lengths, transposed_out=True, skip_lengths=g.lengths)
        if self._trace is not None:
            self._trace.append(('mel_projection', f'{pre}.projection.linear_layer', x, None, g.lengths, mel))
        return mel, (blocks, x)

    def _forward(self, inputs, train, save, bounds=None):
        symbols, durations_float, durations_int, symbols_energy, symbols_pitch, input_lengths, \
            frames_energy, frames_pitch, mel_specs, output_lengths, speaker_ids = inputs
        ops.H.require_gpu(symbols, mel_specs)
        self._step_id += 1
        self._site = 0
        # grouped micro-batches (`data_loader.GroupedBatch`): bounds = per-utterance hard sequence ends of the input and output lengths
        g_out = _Geometry(self, output_lengths, mel_specs.shape[2], None if bounds is None else bounds[2:])
        g_in = _Geometry(self, input_lengths, symbols.shape[1], None if bounds is None else bounds[:2])
        self._geometry = (g_out, g_in)
        W = self._weights(need_dgrad=save)
        S = _Saved() if save else None
        emb, films, s_pe = self._prosody_encoder_fwd(W, frames_energy, frames_pitch, mel_specs, speaker_ids, g_out, train, save)
        beside = self._predictor_beside()
        side = self.ensure_side_stream() if beside else None
        # the speaker classifier feeds nothing but the loss either: the launch stream waits for it together with the predictor
        with _Beside(side, self._handoff, 'classifier fwd'):
            logits, s_cls = self._classifier_fwd(emb)
        enc, s_enc = self._phoneme_encoder_fwd(W, symbols, films[0], g_in, train, save)
        with _Beside(side, self._handoff, 'predictor fwd') as fork:
            y, s_pp = self._predictor_fwd(W, enc, films[1], g_in, train, save)
            fork.mark('predictor fwd done')
        T = mel_specs.shape[2]
        dec_in, weights, _, s_gu = self._upsample_fwd(enc, durations_float, durations_int, symbols_energy, symbols_pitch,
                                                      input_lengths, output_lengths, T, save)
        mel, s_dec = self._decoder_fwd(W, dec_in, films[2], g_out, train, save)
        if beside:
            main = torch.cuda.current_stream()
            main.wait_event(self._handoff['predictor fwd done'])
            # allocated on the side stream, consumed on the launch stream (the loss, `last_outputs`, user code): tell the caching allocator
            # (the saved activations stay in `_wgrad_keep` until the streams have joined at the end of the backward pass)
            logits.record_stream(main)
            y.record_stream(main)
        dur, energy, pitch = ops.unstack(y, 3)
        if save:
            S.pe, S.cls, S.enc, S.pp, S.gu, S.dec, S.films, S.symbols, S.input_lengths, S.enc_out, S.x_mel = \
                s_pe, s_cls, s_enc, s_pp, s_gu, s_dec, films, symbols, input_lengths, enc, mel_specs
        return (logits, films, (dur, energy, pitch), mel, weights), S

    def _predictor_beside(self):
        ''' may the predictor run on the weight-gradient stream beside the launch stream (see `overlap_predictor`)?  Not while a step is
            being captured (the capture's fork bookkeeping is `_flush_wgrads`'s), not under a stage trace, not without that stream '''
        ok = bool(self.overlap_predictor and config.WGRAD_SIDE_STREAM and ops.STEP_PTR is None and self._trace is None and
                  self._trace_bwd is None and self._flat is not None and self._flat.is_cuda)
        if ok and self._handoff is None:
            self._handoff = {name: torch.cuda.Event() for name in _HANDOFFS}
        return ok

    def _classifier_bwd(self, S, d_spk, zeros):
        ''' backward of the speaker classifier behind the gradient reversal (`model.py:27-38, 285-292`): parameter gradients; returns
            d_emb = -lambda dL/d(classifier input) (zeros without a speaker loss) '''
        hp, P, G = self.hp, self._P, self._G
        emb, h1, h2 = S.cls
        cl = 'speaker_classifier.classifier'
        if d_spk is not None and self._fused_classifier():
            d_emb = ops.classifier_bwd(d_spk.contiguous(), emb, h1, h2, P[f'{cl}.1.linear_layer.weight'], P[f'{cl}.3.linear_layer.weight'],
                                       P[f'{cl}.5.linear_layer.weight'], float(hp.lambda_reversal), G[f'{cl}.1.linear_layer.weight'],
                                       G[f'{cl}.1.linear_layer.bias'], G[f'{cl}.3.linear_layer.weight'], G[f'{cl}.3.linear_layer.bias'],
                                       G[f'{cl}.5.linear_layer.weight'], G[f'{cl}.5.linear_layer.bias'])
        elif d_spk is not None:
            d_h2 = ops.linear_small_bwd(d_spk.contiguous(), None, h2, P[f'{cl}.5.linear_layer.weight'], G[f'{cl}.5.linear_layer.weight'],
                                        G[f'{cl}.5.linear_layer.bias'])
            d_h1 = ops.linear_small_bwd(d_h2, h2, h1, P[f'{cl}.3.linear_layer.weight'], G[f'{cl}.3.linear_layer.weight'],
                                        G[f'{cl}.3.linear_layer.bias'], relu=True)
            d_emb = ops.linear_small_bwd(d_h1, h1, emb, P[f'{cl}.1.linear_layer.weight'], G[f'{cl}.1.linear_layer.weight'],
                                         G[f'{cl}.1.linear_layer.bias'], relu=True, dx_scale=-float(hp.lambda_reversal))
        else:
            d_emb = zeros(*emb.shape)
        return d_emb

    def _predictor_bwd(self, W, S, d_dur, d_energy, d_pitch, dfilm_pp, d_enc):
        ''' backward of the local prosody predictor (`model.py:549-575`): parameter gradients, FiLM gradients into dfilm_pp; the gradient
            wrt the encoder output is accumulated into d_enc when given, else returned '''
        P, G = self._P, self._G
        saved_pp, pp_x, pp_y = S.pp
        L = S.symbols.shape[1]
        dy = ops.stack([d_dur.float().contiguous(), d_energy.float().contiguous(), d_pitch.float().contiguous()])
        ppn = 'prosody_predictor'
        dx = ops.linear_small_bwd(dy, None, pp_x, P[f'{ppn}.projection.linear_layer.weight'],
                                  G[f'{ppn}.projection.linear_layer.weight'], G[f'{ppn}.projection.linear_layer.bias'],
                                  mask_lengths=S.input_lengths, N=L)
        for blk in reversed(range(len(saved_pp))):
            s1, s2 = saved_pp[blk]
            dx = self._conv_ln_bwd(W, s2, dx, dfilm=dfilm_pp[:, blk, :])
            if blk == 0 and d_enc is not None:
                return self._conv_ln_bwd(W, s1, dx, dx_out=d_enc)
            dx = self._conv_ln_bwd(W, s1, dx)
        return dx

    # ------------------------------------------------------------------ backward building blocks
    def _wgrad(self, dy, x, dw, db, lengths=None):
        ''' weight / bias gradient on the side stream: these kernels are off the critical path of the backward pass
            (nothing downstream reads dW before the optimizer step), so they overlap with the data-gradient chain. '''
        side = self._side_stream
        if config.SKIP_WGRAD:                           # measurement protocol: what the side-stream work costs the step
            wide = (dy.shape[2] >= 1024) + (x.shape[2] >= 1024)
            if config.SKIP_WGRAD == 1 or (config.SKIP_WGRAD == 2 and wide == 1) or (config.SKIP_WGRAD == 3 and wide == 2) or \
                    (config.SKIP_WGRAD == 4 and dw.dim() == 2):
                return
        if side is None:
            return ops.conv1d_wgrad(dy, x, dw, db, self.cd, lengths)
        # queued: the launches of a whole FFT block (or conv + LayerNorm stage) go out together behind ONE event hop
        # (`_flush_wgrads`) -- an event record + wait per weight gradient cost ~10 us of host time, 54 times per step, in
        # exactly the phoneme-level stretches of the backward pass where the GPU waits for the host
        self._wgrad_pending.append((dy, x, dw, db, lengths))

    def _block_done(self):
        ''' end of an FFT block / conv stage of the backward pass: its queued weight gradients go to the side stream (measured:
            holding the phoneme-level ones back, or flushing every 2 / 4 blocks, is slower -- they run for free exactly where they are) '''
        self._flush_wgrads()

    def _flush_wgrads(self):
        pend, side = self._wgrad_pending, self._side_stream
        if not pend:
            return
        self._wgrad_pending = []
        # the operands were produced on the main stream: one event hop, then launches on the side stream's raw handle with the
        # side stream's own scratch (launches on one stream run in order, so they can share it) -- a
        # `with torch.cuda.stream(side)` block per launch cost 15 us of host time
        self._hop.record()
        side.wait_event(self._hop)
        if ops.STEP_PTR is not None:
            # CAPTURING.  The graph executor keeps the FIRST node recorded behind a fork on the forking node's hardware queue and moves
            # the others to another one: with the weight gradients recorded first, the data-gradient chain hopped queues at every
            # fork and queued up behind weight-gradient kernels (8.57 vs 7.97 ms per replayed step).  So the side-stream launches of
            # this flush are recorded right AFTER the next launch on the launch stream (their dependencies are those of the event
            # hop above either way)
            self._issue_deferred()
            self._side_deferred = pend
            ops.H.AFTER_LAUNCH = self._issue_deferred
            return
        self._issue_side(pend)

    def _issue_deferred(self):
        pend, self._side_deferred = self._side_deferred, None
        ops.H.AFTER_LAUNCH = None
        if pend:
            self._issue_side(pend)

    def _issue_side(self, pend):
        side = self._side_stream
        shape = lambda dy, x, dw: (dy.shape[0], dy.shape[1], x.shape[2], dy.shape[2], dw.shape[2] if dw.dim() == 3 else 1)
        # the weight gradients of one flush over the same rows (an FFT block's four, a conv stage's one) go out as ONE call: their GEMM
        # launches, then a single launch that adds all partial tiles (`ops.conv1d_wgrad_multi`; a reduce launch per weight cost ~20 us
        # of side-stream time each, 54 times per step)
        groups = []
        for it in pend:
            dy, x, dw, db, lengths = it
            key = (dy.shape[0], dy.shape[1], None if lengths is None else lengths.data_ptr())
            if ops.WGRAD_WORKSPACE and groups and groups[-1][0] == key and len(groups[-1][1]) < ops.WGRAD_MULTI_MAX:
                groups[-1][1].append(it)
            else:
                groups.append((key, [it]))
        need = max(sum(ops.wgrad_ws_floats(*shape(dy, x, dw)) for dy, x, dw, db, lengths in items) for _, items in groups)
        if self._wgrad_ws is None or self._wgrad_ws.numel() < need:
            with torch.cuda.stream(side):
                self._wgrad_ws = torch.empty(max(need, 1 << 24), dtype=torch.float32, device=pend[0][0].device)
        probe = ops.PROBE is not None
        for _, items in groups:
            lengths = items[0][4]
            if len(items) > 1 or ops.WGRAD_WORKSPACE:
                call = lambda **kw: ops.conv1d_wgrad_multi([(dy, x, dw, db) for dy, x, dw, db, _ in items], self.cd, lengths, ws=self._wgrad_ws, **kw)
            else:
                dy, x, dw, db, _ = items[0]
                call = lambda **kw: ops.conv1d_wgrad(dy, x, dw, db, self.cd, lengths, ws=self._wgrad_ws, **kw)
            if probe:                                   # bench.py's per-family HIP events must sit on the launch stream
                with torch.cuda.stream(side):
                    call()
            else:
                call(stream=side.cuda_stream)
            # keep the operands alive until the side stream has joined the main one at the end of the backward pass (cheaper on
            # the host than two record_stream calls per launch; the small-N encoder blocks are host-bound)
            for dy, x, dw, db, _ in items:
                self._wgrad_keep.append((dy, x))

    def _fft_stack_bwd(self, W, blocks, du, dfilms):
        ''' backward through a stack of FFT blocks, top block first.  dfilms: (B, nb_blocks, 2C) gradient view or None. '''
        pre = None
        for blk in reversed(range(len(blocks))):
            below = blocks[blk - 1] if blk > 0 else None
            dfilm = dfilms[:, blk, :] if dfilms is not None else None
            dfilm_below = dfilms[:, blk - 1, :] if (dfilms is not None and blk > 0) else None
            du, pre = self._fft_block_bwd(W, blocks[blk], du, dfilm, pre, below, dfilm_below)
        return du

    def _fft_block_bwd(self, W, s, du, dfilm, pre=None, below=None, dfilm_below=None):
        ''' du: grad wrt the block output (fp32).  Returns (grad wrt the block input, pre-computed LN2 backward of the block
            below or None).  dfilm: (B, 2C) view or None.  With bf16 operands the two data-gradient GEMMs that write into
            the residual gradient (FF conv1, QKV projection) carry the backward of the LayerNorm they feed
            (`ops.conv1d_lnbwd`): the attention LayerNorm of this block and the FF LayerNorm of the block below. '''
        P, G, cd = self._P, self._G, self.cd
        a_pre, f_pre = f'{s.pre}.attention', f'{s.pre}.feed_forward'
        lp = cd == torch.bfloat16
        fuse = lp and self.fuse_ln_backward
        if pre is None:
            ds2, dz = ops.layernorm_bwd(du, s.s2, s.mean2, s.rstd2, P[f'{f_pre}.layer_norm.weight'], P[f'{f_pre}.layer_norm.bias'],
                                        G[f'{f_pre}.layer_norm.weight'], G[f'{f_pre}.layer_norm.bias'], film=s.film, dfilm=dfilm,
                                        lengths=s.lengths, p_pre=s.p_conv, seed_pre=s.seeds[2], skip_lengths=s.lengths, lp_only=lp,
                                        separate=True)   # dz is read by the side-stream wgrad while `da` is accumulated in place
        else:
            ds2, dz = pre                                # done in the epilogue of the block above's QKV data gradient
        cap_in = ds2.clone() if self._trace_bwd is not None else None   # dL/d(s2 of this block): the residual gradient is updated in place below
        da = ds2
        self._wgrad(dz, s.h, G[f'{f_pre}.convs.2.conv.weight'], G[f'{f_pre}.convs.2.conv.bias'], s.lengths)
        dh = ops.conv1d(dz, W[f'T:{f_pre}.convs.2.conv.weight'], None, out_dtype=cd, relu_gate=s.hbits if s.hbits is not None else s.h, skip_lengths=s.geo.skip,
                        w_frag=W.get(f'FT:{f_pre}.convs.2.conv.weight'))
        self._wgrad(dh, s.a, G[f'{f_pre}.convs.0.conv.weight'], G[f'{f_pre}.convs.0.conv.bias'], s.lengths)
        mha = f'{a_pre}.multi_head_attention'
        d_o = None
        if fuse:
            # (+ the data gradient of the attention output projection, a 128 -> 128 linear map on the rows this launch produces)
            dproj, d_o = ops.conv1d_lnbwd(dh, W[f'T:{f_pre}.convs.0.conv.weight'], da, s.s1, s.mean1, s.rstd1,
                                          P[f'{a_pre}.layer_norm.weight'], P[f'{a_pre}.layer_norm.bias'], s.lengths,
                                          G[f'{a_pre}.layer_norm.weight'], G[f'{a_pre}.layer_norm.bias'], p_pre=s.p_attn, seed_pre=s.seeds[1],
                                          plan=s.geo.plan, w_frag=W.get(f'FT:{f_pre}.convs.0.conv.weight'),
                                          w2_packed=W[f'T:{mha}.out_proj.weight'])
            ds1 = da
        else:
            ops.conv1d(dh, W[f'T:{f_pre}.convs.0.conv.weight'], None, out=da, accumulate=True, skip_lengths=s.lengths)
            ds1, dproj = ops.layernorm_bwd(da, s.s1, s.mean1, s.rstd1, P[f'{a_pre}.layer_norm.weight'], P[f'{a_pre}.layer_norm.bias'],
                                           G[f'{a_pre}.layer_norm.weight'], G[f'{a_pre}.layer_norm.bias'], lengths=s.lengths,
                                           p_pre=s.p_attn, seed_pre=s.seeds[1], skip_lengths=s.lengths, lp_only=lp, separate=True)
        dx = ds1
        self._wgrad(dproj, s.o, G[f'{mha}.out_proj.weight'], G[f'{mha}.out_proj.bias'], s.lengths)
        if d_o is None:
            d_o = ops.conv1d(dproj, W[f'T:{mha}.out_proj.weight'], None, out_dtype=cd, skip_lengths=s.lengths)
        dqkv = ops.attention_bwd(s.qkv, s.o, d_o, s.lse, s.lengths, s.cfg['attn_nb_heads'], s.p_attn, s.seeds[0], order=s.geo.order)
        self._wgrad(dqkv, s.x, G[f'{mha}.in_proj_weight'], G[f'{mha}.in_proj_bias'], s.lengths)
        if fuse and below is not None:
            fb = f'{below.pre}.feed_forward'
            dz_below = ops.conv1d_lnbwd(dqkv, W[f'T:{mha}.in_proj_weight'], dx, below.s2, below.mean2, below.rstd2,
                                        P[f'{fb}.layer_norm.weight'], P[f'{fb}.layer_norm.bias'], below.lengths,
                                        G[f'{fb}.layer_norm.weight'], G[f'{fb}.layer_norm.bias'], film=below.film, dfilm=dfilm_below,
                                        p_pre=below.p_conv, seed_pre=below.seeds[2])
            self._block_done()
            if self._trace_bwd is not None:              # dx = dL/d(s2 of the block below): its LayerNorm backward ran in the launch above
                self._trace_bwd.append(('fft_block', s, below, cap_in, dx.clone()))
            return dx, (dx, dz_below)
        ops.conv1d(dqkv, W[f'T:{mha}.in_proj_weight'], None, out=dx, accumulate=True, skip_lengths=s.lengths)
        self._block_done()
        if self._trace_bwd is not None:                  # dx = dL/d(block input)
            self._trace_bwd.append(('fft_block', s, None, cap_in, dx.clone()))
        return dx, None

    def _conv_ln_bwd(self, W, s, dy, dfilm=None, need_dx=True, dx_out=None):
        ''' backward of `_conv_ln_fwd`; returns grad wrt its input (dtype = the input's) '''
        P, G = self._P, self._G
        # dc only feeds GEMMs (weight and data gradient): emit it in the MFMA operand type (= rounding at operand load)
        d_dtype = self.cd if (self.cd == torch.bfloat16 and dy.dtype == torch.float32 and s.c.dtype == torch.float32) else s.c.dtype
        dc, _ = ops.layernorm_bwd(dy, s.c, s.mean, s.rstd, P[f'{s.ln_name}.weight'], P[f'{s.ln_name}.bias'],
                                  G[f'{s.ln_name}.weight'], G[f'{s.ln_name}.bias'], film=s.film, dfilm=dfilm, lengths=s.lengths,
                                  d_dtype=d_dtype, p_post=s.p, seed_post=s.seed, relu_input=True, skip_lengths=s.skip)
        if not need_dx:   # last op of the backward pass: nothing left on the main stream to overlap with, and the side stream
            # still has the previous (large) weight gradient queued -- launch here
            ops.conv1d_wgrad(dc, s.x, G[f'{s.conv_name}.conv.weight'], G[f'{s.conv_name}.conv.bias'], self.cd, s.wgrad_lengths)
            if self._trace_bwd is not None:
                self._trace_bwd.append(('conv_ln', s, None, dy.clone(), None))     # no data gradient: the input needs none
            return None
        self._wgrad(dc, s.x, G[f'{s.conv_name}.conv.weight'], G[f'{s.conv_name}.conv.bias'], s.wgrad_lengths)
        self._block_done()
        if dx_out is not None:
            if self._trace_bwd is not None:
                self._trace_bwd.append(('conv_ln', s, None, dy.clone(), None))     # the data gradient is accumulated into dx_out: not separable
            return ops.conv1d(dc, W[f'T:{s.conv_name}.conv.weight'], None, out=dx_out, accumulate=True, skip_lengths=s.skip)
        dx = ops.conv1d(dc, W[f'T:{s.conv_name}.conv.weight'], None, out_dtype=s.x.dtype, skip_lengths=s.skip,
                        w_frag=W.get(f'FT:{s.conv_name}.conv.weight'),
                        wide_plan=s.geo.wide if f'FT:{s.conv_name}.conv.weight' in W else None)
        if self._trace_bwd is not None:
            self._trace_bwd.append(('conv_ln', s, None, dy.clone(), dx.clone()))
        return dx

    def ensure_side_stream(self):
        ''' the weight-gradient stream (created once, with the launch stream of the first backward pass current) '''
        if self._side is None:
            # a stream on ANOTHER hardware queue than the launch stream (probed, `streams.pick`: after RCCL has taken its streams from
            # torch's pool the next pool stream can share the launch stream's queue, and the weight gradients would run in line)
            self._side = streams.pick([torch.cuda.current_stream()], what='weight-gradient stream')
            self._hop = torch.cuda.Event()
        return self._side

    def _backward(self, S, d_spk, d_dur, d_energy, d_pitch, d_mel, d_mel_is_bt=False, section_done=None):
        ''' hand-written backward pass: accumulates every parameter gradient into the flat gradient buffer.
            d_mel: (B, n_mel, T) like the output, or (B, T, n_mel) when d_mel_is_bt.
            section_done(name): called as soon as every gradient of a top-level module is final, in reverse
            registration order (frame_decoder first) -- the data-parallel reducer launches that slice's all-reduce. '''
        use_side = config.WGRAD_SIDE_STREAM
        if use_side:
            self.ensure_side_stream()
        self._side_stream = self._side if use_side else None

        def done(name, last=False):
            ''' a top-level module's gradients are complete once BOTH streams have passed this point.  The compute stream
                must not stall for that (measured: ~60 us of idle main stream per section): the data-parallel hook is issued
                from the side stream after it has caught up with the main stream, so the collective orders itself behind
                both; only the end of the backward pass joins the side stream into the main one (optimizer next). '''
            side = self._side_stream
            self._flush_wgrads()
            if section_done is not None or last:
                self._issue_deferred()                # (capturing: nothing may stay queued across a hook or the final join)
            if section_done is not None:
                if side is not None:
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        section_done(name)
                else:
                    section_done(name)
            if last and side is not None:
                torch.cuda.current_stream().wait_stream(side)
                self._wgrad_keep.clear()            # freed on the main stream, which is now behind every side-stream read
        hp, P, G = self.hp, self._P, self._G
        W = self._packed
        dev = S.enc_out.device
        B, L = S.symbols.shape
        zeros = lambda *shape: ops.zeros(shape, dev)
        layout = film_layout(hp)
        sizes = [B * nb * 2 * ch for nb, ch in layout]                  # the FiLM gradient accumulators of the three stacks: one buffer, one fill
        dfilm_all = zeros(sum(sizes))
        dfilms = [v.view(B, nb, 2 * ch) for v, (nb, ch) in zip(torch.split(dfilm_all, sizes), layout)]
        # ---- local prosody predictor, on the weight-gradient stream beside everything up to the phoneme encoder (see `overlap_predictor`)
        d_enc_pp, beside = None, d_dur is not None and self._side_stream is not None and self._predictor_beside()
        main, side, ev = torch.cuda.current_stream(), self._side_stream if beside else None, self._handoff
        if beside:
            with _Beside(side, ev, 'predictor bwd') as fork:           # the loss gradients and the zeroed FiLM accumulators are in place
                d_enc_pp = self._predictor_bwd(W, S, d_dur, d_energy, d_pitch, dfilms[1], None)
                fork.mark('predictor bwd done')
                # the speaker classifier's backward needs the loss gradient only as well (its d_emb is consumed by the FiLM head far below)
                d_emb_side = self._classifier_bwd(S, d_spk, zeros)
                fork.mark('classifier bwd done')
            self._wgrad_keep.append((d_enc_pp, d_emb_side))             # (read by the launch stream: stay allocated until the streams have joined)
        # ---- decoder
        blocks, dec_x = S.dec
        pre = 'frame_decoder'
        if d_mel is None:
            d_dec = zeros(*dec_x.shape)
        else:
            d_mel_bt = d_mel if d_mel_is_bt else ops.transpose_last2(d_mel.contiguous())
            wname = f'{pre}.projection.linear_layer'
            self._wgrad(d_mel_bt, dec_x, G[f'{wname}.weight'], G[f'{wname}.bias'], S.gu.output_lengths)
            self._flush_wgrads()
            d_dec = ops.conv1d(d_mel_bt, W[f'T:{wname}.weight'], None, out_dtype=torch.float32, skip_lengths=S.gu.output_lengths)
        d_dec = self._fft_stack_bwd(W, blocks, d_dec, dfilms[2])
        done('frame_decoder')
        # ---- Gaussian upsampling (ground-truth durations / energy / pitch: no gradient into the predictor here)
        g = S.gu
        GP = self._gu_params()
        dxp, drin, dr = ops.gu_upsample_bwd(d_dec, g.xp, g.weights, g.means, g.ranges, g.r_pre, GP['w_range'], g.input_lengths,
                                            g.output_lengths)
        gu = 'gaussian_upsampling'
        with _Beside(side, ev, 'upsampler grads'):      # three launches that produce parameter gradients only: nothing downstream waits for them
            ops.linear_small_bwd(dr.unsqueeze(2), None, g.rin, GP['w_range'], G[f'{gu}.projection.0.linear_layer.weight'],
                                 G[f'{gu}.projection.0.linear_layer.bias'], need_dx=False)
            ops.scalar_embed_bwd(drin, [g.durations_float], [G[f'{gu}.duration_projection.conv.weight']],
                                 [G[f'{gu}.duration_projection.conv.bias']])
            ops.scalar_embed_bwd(dxp, [g.energies, g.pitch],
                                 [G[f'{gu}.energy_projection.conv.weight'], G[f'{gu}.pitch_projection.conv.weight']],
                                 [G[f'{gu}.energy_projection.conv.bias'], G[f'{gu}.pitch_projection.conv.bias']])
        if beside:
            self._wgrad_keep.append((dxp, drin, dr))                    # read on the side stream; dxp is NOT modified below (the sum goes into d_enc_pp)
        d_enc = dxp
        done('gaussian_upsampling')
        # ---- local prosody predictor
        if beside:
            main.wait_event(ev['predictor bwd done'])
            d_enc = ops.add_(d_enc_pp, dxp)                             # (into the predictor's buffer: the side stream may still be reading dxp)
        elif d_dur is not None:
            self._predictor_bwd(W, S, d_dur, d_energy, d_pitch, dfilms[1], d_enc)
        done('prosody_predictor')
        # ---- phoneme encoder
        d_enc = self._fft_stack_bwd(W, S.enc, d_enc, dfilms[0])
        with _Beside(side, ev, 'embedding grad'):                      # a parameter gradient only: side stream
            ops.embed_pos_bwd(S.symbols, d_enc, S.input_lengths, G['phoneme_encoder.symbols_embedding.weight'])
        if beside:
            self._wgrad_keep.append(d_enc)
        done('phoneme_encoder')
        # ---- speaker classifier (+ gradient reversal, model.py:27-38)
        pe = S.pe
        if beside:
            main.wait_event(ev['classifier bwd done'])
            d_emb = d_emb_side
        else:
            d_emb = self._classifier_bwd(S, d_spk, zeros)
        done('speaker_classifier')
        # ---- FiLM head
        pre = 'prosody_encoder'
        dpost = G[f'{pre}.post_multipliers'] if pe.post is not None else None
        if ops.USE_FUSED_HEADS:      # two launches: data side (into d_emb, the speaker-embedding gradient, dpost) + all four parameter gradients
            ops.film_head_bwd(pe.g_raw, pe.b_raw, pe.post, pe.z, pe.speaker_ids, P[f'{pre}.gammas_predictor.linear_layer.weight'],
                              P[f'{pre}.betas_predictor.linear_layer.weight'], dfilms, d_emb, G[f'{pre}.spk_embedding.weight'], dpost,
                              G[f'{pre}.gammas_predictor.linear_layer.weight'], G[f'{pre}.gammas_predictor.linear_layer.bias'],
                              G[f'{pre}.betas_predictor.linear_layer.weight'], G[f'{pre}.betas_predictor.linear_layer.bias'], pe.nb, pe.ch)
        else:
            dg_raw, db_raw = ops.film_assemble_bwd(pe.g_raw, pe.b_raw, pe.post, dfilms, dpost, pe.nb, pe.ch)
            dz = ops.linear_small_bwd(dg_raw, None, pe.z, P[f'{pre}.gammas_predictor.linear_layer.weight'],
                                      G[f'{pre}.gammas_predictor.linear_layer.weight'], G[f'{pre}.gammas_predictor.linear_layer.bias'])
            dz2 = ops.linear_small_bwd(db_raw, None, pe.z, P[f'{pre}.betas_predictor.linear_layer.weight'],
                                       G[f'{pre}.betas_predictor.linear_layer.weight'], G[f'{pre}.betas_predictor.linear_layer.bias'])
            ops.add_(dz, dz2)
            ops.gather_add_bwd(dz, pe.speaker_ids, G[f'{pre}.spk_embedding.weight'])
            ops.add_(d_emb, dz)
        # ---- prosody encoder trunk
        dx = ops.masked_mean_bwd(d_emb, pe.output_lengths, pe.T)
        dx = self._fft_stack_bwd(W, pe.blocks, dx, None)
        done('prosody_encoder.trunk')     # blocks, speaker embedding, FiLM projections: final
        # rows >= length of dx are exactly zero (masked LayerNorm rows carry no gradient; pad queries / keys get zero
        # attention gradients), so the gradient wrt the prenet output is dx itself: no masked copy
        ops.scalar_embed_bwd(dx, [pe.frames_energy, pe.frames_pitch],
                             [G[f'{pre}.energy_embedding.conv.weight'], G[f'{pre}.pitch_embedding.conv.weight']],
                             [G[f'{pre}.energy_embedding.conv.bias'], G[f'{pre}.pitch_embedding.conv.bias']],
                             lengths=pe.output_lengths, need_dbase=False)
        dl3 = dx
        dl2 = self._conv_ln_bwd(W, pe.c3, dl3)
        dl1 = self._conv_ln_bwd(W, pe.c2, dl2)
        self._conv_ln_bwd(W, pe.c1, dl1, need_dx=False)
        done('prosody_encoder.prenet', last=True)

    # ------------------------------------------------------------------ fused training step (no autograd graph)
    # gradient sections in registration (= flat buffer) order; the backward pass reports them in REVERSE.  The prosody encoder
    # (half of the parameters) is split where its gradients become final at different times: its FFT blocks, speaker embedding
    # and FiLM projections are done once the trunk's backward has run, the pre-net convolutions (plus the three small tensors
    # registered in front of them) only at the very end -- so only 15 MB, not 30 MB, of all-reduce is left without backward work
    # to hide under.
    SECTIONS = ('prosody_encoder.prenet', 'prosody_encoder.trunk', 'speaker_classifier', 'phoneme_encoder', 'prosody_predictor',
                'gaussian_upsampling', 'frame_decoder')

    def section_slices(self):
        ''' {section: (offset, numel)} in the flat parameter / gradient buffers (registration order) '''
        out = {}
        for name, _, _ in self._table:
            off, n = self._offsets[name]
            sec = name.split('.')[0]
            if sec == 'prosody_encoder':
                tail = name.split('.')[1] in ('blocks', 'spk_embedding', 'gammas_predictor', 'betas_predictor')
                sec = 'prosody_encoder.trunk' if tail else 'prosody_encoder.prenet'
            lo, cnt = out.get(sec, (off, 0))
            assert lo + cnt == off, f'section {sec} is not contiguous at {name}'
            out[sec] = (lo, cnt + n)
        return out

    @torch.no_grad()
    def forward_backward(self, inputs, targets, loss_weights, grad_scale=1., section_done=None, bounds=None):
        ''' forward + 7-term loss + hand-written backward in one call: the body of `train.py:377-391` without an
            autograd graph or host sync.  Gradients accumulate into `flat_gradients()`.  bounds: the per-utterance hard sequence
            ends of a grouped step (`data_loader.GroupedBatch.bounds`): the one pass then equals the reference's accumulation over
            the group's micro-batches (`train.py:379-401`).  Returns the (8,) device
            tensor [speaker, post_mult, duration, energy, pitch, mel_l1, mel_l2, total] (unscaled). '''
        (logits, films, (dur, energy, pitch), mel, weights), S = self._forward(inputs, True, True, bounds=bounds)
        dur_t, energy_t, pitch_t, mel_t, spk_ids = targets
        B, n_mel, T = mel.shape
        g = {'d_dur': torch.empty_like(dur), 'd_energy': torch.empty_like(energy), 'd_pitch': torch.empty_like(pitch),
             'd_mel': torch.empty((B, T, n_mel), dtype=torch.float32, device=mel.device), 'd_spk': torch.empty_like(logits)}
        post = self._P['prosody_encoder.post_multipliers'] if self.hp.post_mult_weight != 0. else None
        d_post = self._G['prosody_encoder.post_multipliers'] if post is not None else None
        terms = ops.loss_fwd_bwd(dur, energy, pitch, dur_t, energy_t, pitch_t, inputs[5], mel, mel_t, inputs[9], logits, spk_ids,
                                 post, loss_weights, grads=g, d_post_mult=d_post, grad_scale=grad_scale, d_mel_transposed=True)
        self._backward(S, g['d_spk'], g['d_dur'], g['d_energy'], g['d_pitch'], g['d_mel'], d_mel_is_bt=True,
                       section_done=section_done)
        self.last_outputs = (logits, films, (dur, energy, pitch), mel, weights)
        return terms

    # ------------------------------------------------------------------ inference (`model.py:789-923`)
    def get_int_durations(self, duration_preds, hparams, dur_factors=None, frame_exact=None):
        ''' `model.py:789-812` on the device: thresholds `duration_preds` in place, returns (duration_preds, durations_int).
            Raises IndexError like the reference when an utterance is shorter than one analysis window.
            frame_exact (an extension): None, or (exact, targets, input_lengths) as `ops.prosody_impose` left them: the
            rows with exact == 1 then get the targets' frames behind K16 (`dx_prosody_impose_durations`; those rows never raise K16's
            IndexError), read back with the same one status copy. '''
        dint, totals, status = ops.int_durations(duration_preds, hparams, dur_factors)
        if frame_exact is not None:
            exact, targets, input_lengths = frame_exact
            ops.prosody_impose_durations(exact, targets, input_lengths, duration_preds, dint, totals, status, hparams)
        st = status.cpu()
        if bool((st == 1).any()):
            raise IndexError('list index out of range')   # extract_features.py:90 / 104
        if bool((st == 2).any()):
            raise RuntimeError('shape mismatch: durations and non-zero symbols differ in number')   # model.py:808
        if frame_exact is not None and bool((st == 3).any()):
            raise ValueError(f'prosody targets: the duration targets of rows {torch.nonzero(st == 3).flatten().tolist()} sum to 0 frames')
        if frame_exact is not None and bool((st == 4).any()):
            raise ValueError(f'prosody targets: rows {torch.nonzero(st == 4).flatten().tolist()} have a weight outside [0, 1]')
        self._last_totals = totals
        return duration_preds, dint

    def _speaker_stats(self, hparams, device):
        n = max(int(k.split(' ')[1]) for k in hparams.stats if k.startswith('spk ')) + 1 if hparams.stats else 0
        n = max(n, int(self.hp.n_speakers))   # ids below n_speakers without statistics read (0, 1) instead of out of bounds
        mean, std = torch.zeros(max(n, 1)), torch.ones(max(n, 1))
        for k, v in hparams.stats.items():
            if k.startswith('spk '):
                mean[int(k.split(' ')[1])], std[int(k.split(' ')[1])] = v['pitch']['mean'], v['pitch']['std']
        return mean.to(device), std.to(device)

    def pitch_shift(self, pitch_preds, pitch_factors, hparams, speaker_ids):
        ''' `model.py:814-834` (in place) '''
        mean, std = self._speaker_stats(hparams, pitch_preds.device)
        ones = torch.ones_like(pitch_preds)
        ops.prosody_control(ones.clone(), pitch_preds, ones, pitch_factors.contiguous(), torch.ones_like(pitch_preds, dtype=torch.long),
                            0, speaker_ids, mean, std)
        return pitch_preds

    def pitch_multiply(self, pitch_preds, pitch_factors):
        ''' `model.py:836-864` (in place) '''
        ones = torch.ones_like(pitch_preds)
        ops.prosody_control(ones.clone(), pitch_preds, ones, pitch_factors.contiguous(), torch.ones_like(pitch_preds, dtype=torch.long), 1)
        return pitch_preds

    @torch.no_grad()
    def inference(self, inputs, pitch_transform, hparams, prosody_targets=None):
        ''' `model.py:866-923`.  prosody_targets (an extension): None, or a `clone.ProsodyTargets` in standardised units
            whose rows are the batch's: per-symbol durations (frames), energies and pitches imposed on the predictor's outputs before
            the factors, the integer durations and the pitch transform.  `self.last_frame_exact` is then the (B,) int32 device
            tensor of the rows whose integer durations ARE the targets, and None after a call without targets.  With None nothing
            else is launched or allocated. '''
        symbols, dur_factors, energy_factors, pitch_factors, input_lengths, \
            energy_refs, pitch_refs, mel_spec_refs, ref_lengths, speaker_ids = inputs
        if pitch_transform not in ('add', 'multiply'):
            raise NotImplementedError
        ops.H.require_gpu(symbols, mel_spec_refs)
        self._site = 0
        W = self._weights(need_dgrad=False)
        g_ref = _Geometry(self, ref_lengths, mel_spec_refs.shape[2])
        g_in = _Geometry(self, input_lengths, symbols.shape[1])
        self._geometry = (g_ref, g_in)
        _, films, _ = self._prosody_encoder_fwd(W, energy_refs, pitch_refs, mel_spec_refs, speaker_ids, g_ref, False, False)
        enc, _ = self._phoneme_encoder_fwd(W, symbols, films[0], g_in, False, False)
        y, _ = self._predictor_fwd(W, enc, films[1], g_in, False, False)
        dur, energy, pitch = ops.unstack(y, 3)
        self.last_frame_exact = None      # (of THIS call: never the flags of an earlier one)
        if prosody_targets is None:
            dur, dur_int = self.get_int_durations(dur, hparams, dur_factors.contiguous())
        else:
            if prosody_targets.units != 'standardised':
                raise ValueError("inference takes prosody targets in standardised units: see ProsodyTargets.standardised")
            dur_factors = dur_factors.contiguous()
            exact = ops.prosody_impose(dur, energy, pitch, prosody_targets, input_lengths, dur_factors, hparams)
            dur, dur_int = self.get_int_durations(dur, hparams, dur_factors, (exact, prosody_targets, input_lengths))
            self.last_frame_exact = exact
        if pitch_transform == 'add':
            mean, std = self._speaker_stats(hparams, dur.device)
            ops.prosody_control(energy, pitch, energy_factors.contiguous(), pitch_factors.contiguous(), dur_int, 0, speaker_ids, mean, std)
        else:
            ops.prosody_control(energy, pitch, energy_factors.contiguous(), pitch_factors.contiguous(), dur_int, 1)
        output_lengths = self._last_totals
        T = int(output_lengths.max())   # the one host sync of the synthesis path: sizes the output
        g_out = _Geometry(self, output_lengths, T)
        self._geometry += (g_out,)
        dec_in, weights, _, _ = self._upsample_fwd(enc, dur, dur_int, energy, pitch, input_lengths, output_lengths, T, False)
        assert dec_in.size(1) == T   # model.py:914
        mel, _ = self._decoder_fwd(W, dec_in, films[2], g_out, False, False)
        return [dur, dur_int, energy, pitch, input_lengths], [mel, output_lengths], weights
