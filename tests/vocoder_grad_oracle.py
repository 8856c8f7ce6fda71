"""Float64 gradients of the HiFi-GAN generator's layers and of the whole generator: torch autograd through tests/vocoder_oracle.py
(`conv` / `upsample` / `generator`, masks on), imported unchanged -- the reference every vocoder-training test compares with, never
the code under test.  Pinned against plain-Python loops in tests/test_vocoder_train_host.py.

The bf16 mode (`rounding=True`) rounds what the kernels round: the oracle's forward already rounds the weights and each conv's
post-activation input; here a `round_grad` identity sits on each convolution's output BEFORE the bias, and its backward rounds the
incoming gradient to bf16.  So dW = rnd(dy)^T rnd(f(x)), dx = gate * rnd(W)^T rnd(dy), and the bias gradient sums the unrounded dy.
conv_post is exempt, as in the forward.  Layout is torch's (B, C, T)."""
import contextlib

import torch

from tests import vocoder_oracle as O


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.float().to(torch.bfloat16).to(g.dtype)


def round_grad(x, rounding):
    return _RoundGrad.apply(x) if rounding else x


class _RoundOperand(torch.autograd.Function):
    ''' `vocoder_oracle.rnd` with a straight-through backward: autograd through rnd's dtype casts would round the GRADIENT of the
        operand to bf16 as well, which no kernel does (dW and dx leave the MFMA as fp32 sums) '''
    @staticmethod
    def forward(ctx, x):
        return O.rnd(x, True)

    @staticmethod
    def backward(ctx, g):
        return g


def round_operand(x, rounding):
    return _RoundOperand.apply(x) if rounding else x


_conv, _upsample = O.conv, O.upsample


def conv(x, w, b, dilation, n, slope=0.1, masks=True, rounding=False):
    ''' `vocoder_oracle.conv` (the same forward values as with its own `rounding`) with the operands rounded straight-through and
        the gradient rounding between the convolution and its bias '''
    xa, wr = round_operand(O.lrelu(x, slope), rounding), round_operand(w.to(x.dtype), rounding)
    y = round_grad(_conv(xa, wr, torch.zeros_like(b), dilation, n, slope=1., masks=False, rounding=False), rounding)
    y = y + b.to(x.dtype)[None, :, None]
    return O.mask_rows(y, n) if masks else y


def upsample(x, w, b, u, n, slope=0.1, masks=True, rounding=False):
    xa, wr = round_operand(O.lrelu(x, slope), rounding), round_operand(w.to(x.dtype), rounding)
    y = round_grad(_upsample(xa, wr, torch.zeros_like(b), u, n, slope=1., masks=False, rounding=False), rounding)
    y = y + b.to(x.dtype)[None, :, None]
    return O.mask_rows(y, n * u) if masks else y


@contextlib.contextmanager
def _rounded_gradients():
    ''' `vocoder_oracle.generator` calls the module's `conv` / `upsample`: for the span of one call they are the two above '''
    O.conv, O.upsample = conv, upsample
    try:
        yield
    finally:
        O.conv, O.upsample = _conv, _upsample


def conv_grads(x, w, b, dilation, n, dy, slope=0.1, rounding=False, dtype=torch.float64):
    ''' (dx, dw, db) of sum(conv(x) * dy); x (B, Cin, T), dy (B, Cout, T) '''
    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = conv(x, w, b, dilation, n, slope=slope, rounding=rounding)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), (x, w, b))


def upsample_grads(x, w, b, u, n, dy, slope=0.1, rounding=False, dtype=torch.float64):
    ''' (dx, dw, db) of sum(upsample(x) * dy); x (B, Cin, T), dy (B, Cout, T u), w (Cin, Cout, k) '''
    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = upsample(x, w, b, u, n, slope=slope, rounding=rounding)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), (x, w, b))


def normed(g, v):
    ''' weight norm over every axis but 0 '''
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


def generator_grads(cfg, sd, mel, lengths, proj, rounding=False, dtype=torch.float64):
    ''' sd: a weight-norm state dict (`<layer>.weight_g` / `.weight_v` / `.bias`); loss = sum(generator(mel) * proj).
        Returns (waveform, {parameter name: gradient}, gradient of the mel), all in `dtype` '''
    params = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    mel = mel.detach().to(dtype).requires_grad_(True)
    weights = {name: (normed(params[f'{name}.weight_g'], params[f'{name}.weight_v']), params[f'{name}.bias'])
               for name, _, _, _ in O.layer_shapes(cfg)}
    with _rounded_gradients():
        wav = O.generator(cfg, weights, mel, lengths, masks=True, rounding=rounding, dtype=dtype)
    names = list(params)
    grads = torch.autograd.grad((wav * proj.to(dtype)).sum(), [params[k] for k in names] + [mel])
    return wav.detach(), dict(zip(names, grads[:-1])), grads[-1]
