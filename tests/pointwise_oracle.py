"""Float64 oracle of csrc/pointwise.hip (scalar-feature embedding, symbol embedding + positions, gather-add, masked mean, FiLM
assembly, the exact-fp32 small linear, column sums) and csrc/heads.hip (FiLM head, speaker classifier) -- in numpy, without autograd
and without a GPU.  tests/test_pointwise_host.py holds it against float64 autograd and its restated launch geometry against the
kernel source; tests/test_gpu_pointwise.py and tests/test_gpu_heads.py hold the kernels against it.

Conventions
  * The inputs are the kernels' fp32 arrays, taken as exact.  Scalars that reach a kernel as `float` (`dx_scale`, `lambda`) are
    rounded to fp32 first.
  * Accumulated outputs -- dw, dbias, dtable, dpost, d_emb and d_spk_table of the FiLM head, the heads' dW / db -- are compared as
    old + contribution: every function here returns the CONTRIBUTION and the sum of the absolute values of its addends, and the
    bound functions take |old| in.
  * Masks as the kernels apply them: a row at or behind its utterance's length contributes nothing and is written as an exact zero
    where the kernel writes it (out of scalar_embed / embed_pos, dbase up to N, y and dx of the masked linear).  The masked mean's
    backward writes dy / len to ALL N rows: the reference's sum runs over the (zero) padding.
  * A zero-length utterance has mean 0 and gradient 0.
  * A relu gate is taken from the forward output the kernel is handed (`y`, `h1`, `h2` are inputs of the backward functions).

Error bounds (u = 2^-24, the unit roundoff of fp32; division is correctly rounded in this build: no fast-math flag; none of these
kernels calls expf or logf, so nothing here is measured)
  * Data movement and single correctly rounded operations are compared bit for bit against the same operation in numpy fp32:
    embed_pos and gather_add forward (one addition), transpose_last2 (bf16 = round to nearest even), stack / unstack, add_,
    fill_zero, the masked mean's backward (one division), dg_raw / db_raw / beta of the FiLM assembly (one product), every masked
    or dead row (exact zero), every row an atomic kernel does not address (keeps its bits).
  * A sum or dot product is bounded by gamma(K) = K u / (1 - K u) times the sum of the ABSOLUTE values of its addends (the old
    value of an accumulated output among them), K the number of roundings the longest path of an addend goes through.  A
    multiply-add may or may not be contracted: the bound takes the uncontracted form, where the product is rounded once before
    its chain of additions ("+ 1 (product)" below).  K from the launch geometry restated below:
        scalar_embed_fwd     nfeat (taps + 1) + base + pos terms, one rounding each at most        (`se_fwd_terms`; <= 3 * 4 + 2)
        scalar_embed_bwd     ceil(rows_per_block / 8) trips of a row lane + 1 (product) + 3 (8-lane tree) + one atomic per slab
                             and utterance landing on the address                                  (`se_bwd_chain`)
        masked_mean_fwd      ceil(len / 8) trips + 8 lane partials + 1 (division)                  (`mean_chain`)
        embed_pos_bwd / gather_add_bwd   one atomic per valid position naming the row
        film_assemble_fwd    gamma = post g + 1: 2
        dpost                1 (product) + 6 butterfly steps where a wave reduces + the atomics landing on the block: one per
                             wave whose live lanes share a block, one per lane otherwise             (`film_landings`, `head_landings`)
        linear_small_fwd, dot128   K multiply-adds + 1 (product) + the bias: K + 2
        linear_small_bwd_dx  o_chunk multiply-adds + 1 (product) + 1 (scale) + `chunks` atomics when chunks > 1  (`ls_dx_chain`)
        linear_small_bwd_dw  rows_per_chunk / 4 trips + 3 (tail rows) + 1 (product) + 2 (4-way tree) + one atomic per chunk
        linear_rows_bwd_dw   M multiply-adds + 1 (product) + 1 atomic                              (`ls_dw_chain` for both)
        heads_dw             ceil(B / 2) multiply-adds + 1 (product) + 2 (s0 + s1, +=) + 1 (the stored dg_raw / g1 / g2 is rounded)
        film_head_bwd_dx     2 ncol multiply-adds + 1 (product) + 1 (dg_raw) + ceil(W / 128) atomics on d_emb, times the utterances that share
                             the speaker id on d_spk_table                                          (`head_dx_chain`)
        colsum               rows_per_block additions + one atomic per row block
  * Where one thread adds in a KNOWN order -- the dot products of linear_small_fwd / dot128 (k ascending, the bias last),
    classifier_bwd_dx (o ascending), the 128-column walk of film_head_bwd_dx (gamma and beta interleaved) and the row walk of
    linear_rows_bwd_dw -- the K u sum |addends| above overestimates sums of mixed sign by about sqrt(K), and the running bound
    replaces it: the error of acc_i = fl(acc_{i-1} + p_i) is sum_i delta_i (acc_{i-1} + p_i), at most u times the sum of the
    absolute PARTIAL sums (`chain_bound`, which also allows each product one rounding of its own).  Atomics that follow keep
    their count times u times (|old| + the sum of the absolute workgroup sums).
  * Chains of layers (classifier, FiLM head forward) propagate: the error of a layer's input times the absolute weights, plus the
    layer's own bound.  A relu is 1-Lipschitz.
"""
from collections import namedtuple

import numpy as np

U32 = 2. ** -24
F = np.float32
C128 = 128


def f32(x):
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


def gamma(K):
    e = K * U32
    return e / (1. - e)


def d(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- launch geometry, restated
SE_MAX_ROWS = 1024          # scalar_embed_bwd_kernel: most rows of a slab
SE_WG_TARGET = 256          # dx_scalar_embed_bwd doubles rows_per_block from 64 while there are more workgroups than this
LS_FEW_ROWS = 512           # dx_linear_small_bwd: unmasked and M <= this -> linear_rows_bwd_dw_kernel (LDS tiles)
LS_DX_OCHUNK, LS_DX_SMALL = 16, 1 << 18     # the dx kernel splits O into chunks of 16 when O > 16 and M * K < 2^18
LS_RPC_MAX, LS_CHUNK_TARGET = 4096, 256     # the generic dw kernel doubles rows_per_chunk from 64 while there are more chunks
LT, LR = 64, 32             # linear_rows_bwd_dw_kernel: output tile, rows per LDS round
HD = 128                    # heads.hip: the embedding width
GRID_CAP = 4096             # grid_for's default cap (256 threads per workgroup)
COLSUM_RPB_MAX, COLSUM_BLOCK_TARGET = 8192, 512
WAVE = 64


def se_rows_per_block(B, N):
    rpb = 64
    while rpb < SE_MAX_ROWS and cdiv(N, rpb) * B > SE_WG_TARGET:
        rpb *= 2
    return rpb


def se_slabs(B, N):
    ''' [(n0, n1)] of the slabs of one utterance '''
    rpb = se_rows_per_block(B, N)
    return [(n0, min(N, n0 + rpb)) for n0 in range(0, N, rpb)]


def se_fwd_terms(nfeat, taps, base, pos):
    return nfeat * (taps + 1) + int(base) + int(pos)


def se_bwd_chain(B, N):
    rpb = se_rows_per_block(B, N)
    return cdiv(rpb, 8) + 1 + 3 + cdiv(N, rpb) * B


def mean_chain(length):
    return cdiv(max(int(length), 0), 8) + 8 + 1


def ls_few_rows(M, masked):
    return (not masked) and M <= LS_FEW_ROWS


def ls_chunks(M, K, O):
    ''' (chunks, o_chunk) of linear_small_bwd_dx_kernel '''
    chunks = cdiv(O, LS_DX_OCHUNK) if (O > LS_DX_OCHUNK and M * K < LS_DX_SMALL) else 1
    return chunks, cdiv(O, chunks)


def ls_rows_per_chunk(M):
    rpc = 64
    while rpc < LS_RPC_MAX and cdiv(M, rpc) > LS_CHUNK_TARGET:
        rpc *= 2
    return rpc


def ls_dx_chain(M, K, O):
    chunks, o_chunk = ls_chunks(M, K, O)
    return o_chunk + 1 + 1 + (chunks if chunks > 1 else 0)


def ls_dw_chain(M, masked):
    if ls_few_rows(M, masked):
        return M + 1 + 1
    rpc = ls_rows_per_chunk(M)
    return rpc // 4 + 3 + 1 + 2 + cdiv(M, rpc)


def ls_chunk_seams(M):
    ''' first rows of the generic dw kernel's chunks behind the first '''
    rpc = ls_rows_per_chunk(M)
    return list(range(rpc, M, rpc))


def colsum_rows_per_block(rows):
    rpb = 64
    while rpb < COLSUM_RPB_MAX and cdiv(rows, rpb) > COLSUM_BLOCK_TARGET:
        rpb *= 2
    return rpb


def colsum_chain(rows):
    rpb = colsum_rows_per_block(rows)
    return min(rows, rpb) + cdiv(rows, rpb)


def film_width(nb, ch):
    return sum(n * c for n, c in zip(nb, ch))


def film_keys(nb, ch):
    ''' per column of the (W) projection axis: (module, block within the module, channel, global block = key) '''
    m_, blk_, c_, key_ = [], [], [], []
    blk0 = 0
    for m in range(3):
        for blk in range(nb[m]):
            for c in range(ch[m]):
                m_.append(m); blk_.append(blk); c_.append(c); key_.append(blk0 + blk)
        blk0 += nb[m]
    return np.array(m_), np.array(blk_), np.array(c_), np.array(key_)


def _landings(keys_per_wave, nblk):
    ''' keys_per_wave: iterable of int arrays (-1 = a lane without a column).  -> (atomics landing per block, waves that reduced,
        lanes that took the per-lane branch) '''
    land = np.zeros(nblk, dtype=np.int64)
    uniform = lanes = 0
    for k in keys_per_wave:
        if (k == k[0]).all():
            if k[0] >= 0:
                land[k[0]] += 1
                uniform += 1
        else:
            live = k[k >= 0]
            np.add.at(land, live, 1)
            lanes += live.size
    return land, uniform, lanes


def film_landings(nb, ch, B):
    ''' film_assemble_bwd_kernel: a wave is 64 consecutive elements of the flattened (B, W) index (256-thread workgroups, grid
        stride a multiple of 256); dead lanes behind B W do not count against uniformity '''
    key = film_keys(nb, ch)[3]
    flat = np.tile(key, B)
    return _landings([flat[i:i + WAVE] for i in range(0, flat.size, WAVE)], int(sum(nb)))


def head_landings(nb, ch, B):
    ''' film_head_bwd_dx_kernel: grid (ceil(W / 128), B) of 128 threads -- a wave is 64 consecutive columns of ONE utterance, and a
        lane behind W (key -1) breaks uniformity '''
    key = film_keys(nb, ch)[3]
    W = key.size
    padded = np.full(cdiv(W, 128) * 128, -1, dtype=np.int64)
    padded[:W] = key
    waves = [padded[i:i + WAVE] for i in range(0, padded.size, WAVE)] * B
    return _landings(waves, int(sum(nb)))


def dpost_chain(landings, reduced):
    return 1 + (6 if reduced else 0) + int(landings.max())


def head_dx_chain(W, sharing=1):
    return 2 * min(W, 128) + 1 + 1 + cdiv(W, 128) * sharing


def heads_dw_chain(B):
    return cdiv(B, 2) + 1 + 2 + 1


def chain_bound(P):
    ''' a chain of fp32 additions in a KNOWN order, acc_i = fl(acc_{i-1} + p_i) with p along the last axis: the error is
        sum_i delta_i (acc_{i-1} + p_i), |delta_i| <= u, so it is bounded by u times the sum of the absolute PARTIAL sums -- which for
        addends of mixed sign is far below K u sum |p|.  The computed partial sums are within gamma(i) sum_{j <= i} |p_j| of the exact
        ones, and every addend is a product that may be rounded once before it is added (not contracted): u sum |p| '''
    P = d(P)
    s, A = np.cumsum(P, axis=-1), np.cumsum(np.abs(P), axis=-1)
    i = np.arange(1, P.shape[-1] + 1)
    return U32 / (1. - U32) * (np.abs(s) + gamma(i) * A).sum(-1) + gamma(2) * A[..., -1]


def acc_bound(K, addends_abs, old=0.):
    ''' bound of old + contribution when `addends_abs` is the sum of the absolute values of the contribution's addends '''
    return gamma(K) * (np.abs(d(old)) + addends_abs)


# ---------------------------------------------------------------------------------------------------- masks
def row_mask(lengths, B, N):
    ''' (B, N) bool: n < len_b (all true without lengths) '''
    if lengths is None:
        return np.ones((B, N), dtype=bool)
    return np.arange(N)[None, :] < np.asarray(lengths).reshape(B, 1)


# ---------------------------------------------------------------------------------------------------- scalar-feature embedding
def _taps_of(x, taps):
    ''' (B, N) -> (taps, B, N): x[n + k - 1] with zeros outside [0, N) for three taps, x itself for one '''
    x = d(x)
    if taps == 1:
        return x[None]
    p = np.pad(x, ((0, 0), (1, 1)))
    return np.stack([p[:, 0:-2], p[:, 1:-1], p[:, 2:]])


def scalar_embed_fwd(feats, ws, biases, base=None, pos=None, lengths=None):
    ''' out[b, n, c] = base + sum_f (sum_k w_f[c, 0, k] x_f[b, n + k - 1] + bias_f[c]) + pos[n, c] for n < len_b, else 0.
        The taps read the FEATURE past the length (only the output row is masked).  -> (out, bound) '''
    B, N = feats[0].shape
    taps = ws[0].shape[2]
    out = np.zeros((B, N, C128))
    mag = np.zeros((B, N, C128))
    for x, w, bias in zip(feats, ws, biases):
        t = _taps_of(x, taps)                                  # (taps, B, N)
        w = d(w)[:, 0, :]                                      # (C, taps)
        out += np.einsum('kbn,ck->bnc', t, w) + d(bias)
        mag += np.einsum('kbn,ck->bnc', np.abs(t), np.abs(w)) + np.abs(d(bias))
    if base is not None:
        out += d(base); mag += np.abs(d(base))
    if pos is not None:
        out += d(pos)[None, :N]; mag += np.abs(d(pos))[None, :N]
    m = row_mask(lengths, B, N)[:, :, None]
    K = se_fwd_terms(len(feats), taps, base is not None, pos is not None)
    return out * m, gamma(K) * mag * m


SeBwd = namedtuple('SeBwd', 'dbase dw dbias aw ab')


def scalar_embed_bwd(dout, feats, taps, lengths=None):
    ''' dbase = dout * mask (all N rows); dw_f[c, 0, k] = sum_{b, n < len_b} dout[b, n, c] x_f[b, n + k - 1]; dbias_f[c] = the same
        sum of dout.  aw / ab: the sums of the absolute values of the addends '''
    B, N, C = dout.shape
    g = d(dout) * row_mask(lengths, B, N)[:, :, None]
    dw, aw = [], []
    for x in feats:
        t = _taps_of(x, taps)
        dw.append(np.einsum('bnc,kbn->ck', g, t)[:, None, :])
        aw.append(np.einsum('bnc,kbn->ck', np.abs(g), np.abs(t))[:, None, :])
    return SeBwd(g, dw, [g.sum((0, 1))] * len(feats), aw, [np.abs(g).sum((0, 1))] * len(feats))


def scalar_embed_bwd_sparse(rows, feats, taps, lengths, B, N):
    ''' the same for a dout that is zero but for `rows` = {(b, n): (C) vector}: -> (dw, dbias, aw, ab, the rows that survive the mask) '''
    live = {bn: d(v) for bn, v in rows.items() if lengths is None or bn[1] < int(lengths[bn[0]])}
    dw = [np.zeros((C128, 1, taps)) for _ in feats]
    aw = [np.zeros((C128, 1, taps)) for _ in feats]
    db, ab = np.zeros(C128), np.zeros(C128)
    for (b, n), v in live.items():
        db += v; ab += np.abs(v)
        for f, x in enumerate(feats):
            for k in range(taps):
                j = n + k - 1 if taps == 3 else n
                if 0 <= j < N:
                    dw[f][:, 0, k] += v * float(x[b, j])
                    aw[f][:, 0, k] += np.abs(v * float(x[b, j]))
    return dw, [db] * len(feats), aw, [ab] * len(feats), live


# ---------------------------------------------------------------------------------------------------- embedding + positions, gather-add
def embed_pos_fwd32(ids, table, pos, lengths):
    ''' fp32, bit for bit: table[id] + pos[n] is one correctly rounded addition; rows at or behind the length are zeros '''
    B, N = ids.shape
    out = (np.asarray(table, dtype=F)[ids] + np.asarray(pos, dtype=F)[None, :N]).astype(F)
    return out * row_mask(lengths, B, N)[:, :, None].astype(F)


def embed_pos_fwd(ids, table, pos, lengths):
    B, N = ids.shape
    return (d(table)[ids] + d(pos)[None, :N]) * row_mask(lengths, B, N)[:, :, None]


def scatter_rows(ids, g, n_rows, valid=None):
    ''' table gradient of a gather: contribution[r] = sum of g over the valid positions with id r; -> (contribution, sum of the
        absolute values, number of addends per row) '''
    ids = np.asarray(ids).reshape(-1)
    g = d(g).reshape(ids.size, -1)
    if valid is not None:
        keep = np.asarray(valid).reshape(-1)
        ids, g = ids[keep], g[keep]
    out, mag = np.zeros((n_rows, g.shape[1])), np.zeros((n_rows, g.shape[1]))
    np.add.at(out, ids, g)
    np.add.at(mag, ids, np.abs(g))
    return out, mag, np.bincount(ids, minlength=n_rows)


def scatter_bound(mag, count, old):
    ''' one atomic per addend on top of the old value '''
    return gamma(np.maximum(count, 1))[:, None] * (np.abs(d(old)) + mag) * (count > 0)[:, None]


def gather_add_fwd32(a, table, ids):
    return (np.asarray(a, dtype=F) + np.asarray(table, dtype=F)[ids]).astype(F)


# ---------------------------------------------------------------------------------------------------- masked mean
def masked_mean_fwd(x, lengths):
    ''' mean over the rows below the length (the kernel reads no other row); 0 for a zero-length utterance.  -> (mean, bound) '''
    B, N, C = x.shape
    out, bound = np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        n = min(int(lengths[b]), N)
        if int(lengths[b]) > 0:
            out[b] = d(x[b, :n]).sum(0) / int(lengths[b])
            bound[b] = gamma(mean_chain(n)) * np.abs(d(x[b, :n])).sum(0) / int(lengths[b])
    return out, bound


def masked_mean_bwd32(dy, lengths, N):
    ''' fp32, bit for bit: dy / (float)len on ALL N rows; zeros for a zero-length utterance '''
    dy = np.asarray(dy, dtype=F)
    B, C = dy.shape
    out = np.zeros((B, N, C), dtype=F)
    for b in range(B):
        if int(lengths[b]) > 0:
            out[b] = (dy[b] / F(int(lengths[b]))).astype(F)[None]
    return out


def masked_mean_bwd(dy, lengths, N):
    B, C = dy.shape
    ln = d(lengths).reshape(B, 1, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(ln > 0, d(dy)[:, None, :] / ln, 0.) * np.ones((1, N, 1))


# ---------------------------------------------------------------------------------------------------- FiLM assembly
def _post_cols(post, nb, ch):
    ''' (pg, pb) per projection column; ones without post-multipliers '''
    key = film_keys(nb, ch)[3]
    if post is None:
        return np.ones(key.size), np.ones(key.size)
    p = d(post).reshape(2, -1)
    return p[0][key], p[1][key]


def _split(cols_g, cols_b, nb, ch):
    ''' (B, W) gamma and beta columns -> [film_m (B, nb_m, 2 ch_m)] '''
    B = cols_g.shape[0]
    films, c0 = [], 0
    for m in range(3):
        w = nb[m] * ch[m]
        films.append(np.concatenate([cols_g[:, c0:c0 + w].reshape(B, nb[m], ch[m]), cols_b[:, c0:c0 + w].reshape(B, nb[m], ch[m])], axis=2))
        c0 += w
    return films


def _unsplit(films, nb, ch):
    B = films[0].shape[0]
    g = np.concatenate([d(films[m])[:, :, :ch[m]].reshape(B, -1) for m in range(3)], axis=1)
    b = np.concatenate([d(films[m])[:, :, ch[m]:].reshape(B, -1) for m in range(3)], axis=1)
    return g, b


def film_assemble_fwd(g_raw, b_raw, post, nb, ch, eg=0., eb=0.):
    ''' gamma = post_g[blk] g_raw + 1, beta = post_b[blk] b_raw, split per (module, block).  eg / eb: error bounds of g_raw / b_raw
        when they are themselves computed.  -> ([film_m], [bound_m]) '''
    pg, pb = _post_cols(post, nb, ch)
    gam, bet = pg * d(g_raw) + 1., pb * d(b_raw)
    e_gam = np.abs(pg) * eg + gamma(2) * (np.abs(pg * d(g_raw)) + 1.)
    e_bet = np.abs(pb) * eb + U32 * np.abs(bet)
    if post is None:                    # 1.f * g is exact: one rounding
        e_gam = eg + U32 * (np.abs(d(g_raw)) + 1.)
        e_bet = eb + 0. * bet
    return _split(gam, bet, nb, ch), _split(e_gam + 0. * gam, e_bet + 0. * bet, nb, ch)


def film_assemble_fwd32(g_raw, b_raw, post, nb, ch):
    ''' what is a single rounding, in fp32: beta always, gamma without post-multipliers '''
    pg, pb = _post_cols(post, nb, ch)
    g_raw, b_raw = np.asarray(g_raw, dtype=F), np.asarray(b_raw, dtype=F)
    bet = (pb.astype(F) * b_raw).astype(F)
    gam = (g_raw + F(1.)).astype(F) if post is None else np.zeros_like(g_raw)
    return _split(gam, bet, nb, ch)


FilmBwd = namedtuple('FilmBwd', 'dg_raw db_raw dpost apost')


def film_assemble_bwd(g_raw, b_raw, post, dfilms, nb, ch):
    ''' dg_raw = dfilm_gamma post_g, db_raw = dfilm_beta post_b (single products); dpost[0][blk] = sum_{b, c} dfilm_gamma g_raw,
        dpost[1][blk] = sum dfilm_beta b_raw (None without post-multipliers) '''
    pg, pb = _post_cols(post, nb, ch)
    dg, db = _unsplit(dfilms, nb, ch)
    if post is None:
        return FilmBwd(dg * pg, db * pb, None, None)
    key, nblk = film_keys(nb, ch)[3], int(sum(nb))
    dpost, apost = np.zeros((2, nblk)), np.zeros((2, nblk))
    for i, t in enumerate((dg * d(g_raw), db * d(b_raw))):
        np.add.at(dpost[i], key, t.sum(0))
        np.add.at(apost[i], key, np.abs(t).sum(0))
    return FilmBwd(dg * pg, db * pb, dpost, apost)


# ---------------------------------------------------------------------------------------------------- exact-fp32 small linear
def dense(x, w, bias, relu=False, ex=0.):
    ''' y = act(x W^T + bias) with the bound of K multiply-adds and the bias; ex: error bound of x.  -> (y, bound) '''
    x, w = d(x), d(w)
    K = x.shape[-1]
    b = 0. if bias is None else d(bias)
    y = x @ w.T + b
    # k ascending, the bias last (linear_small_fwd_kernel, dot128): a chain in a known order
    P = np.concatenate([x[..., None, :] * w, np.broadcast_to(b, y.shape)[..., None]], axis=-1)
    bound = chain_bound(P) + (ex * np.ones_like(x)) @ np.abs(w).T
    return (np.maximum(y, 0.) if relu else y), bound


def linear_small_fwd(x, w, bias, relu=False, mask_lengths=None, N=1):
    ''' x (M, K) or (B, N, K); rows m with m % N >= mask_lengths[m // N] are zeros.  -> (y (M, O), bound) '''
    x = d(x).reshape(-1, x.shape[-1])
    y, bound = dense(x, w, bias, relu)
    if mask_lengths is not None:
        m = row_mask(mask_lengths, x.shape[0] // N, N).reshape(-1, 1)
        y, bound = y * m, bound * m
    return y, bound


LsBwd = namedtuple('LsBwd', 'dx adx dw aw db ab cw cb')


def linear_small_bwd(dy, y, x, w, relu=False, mask_lengths=None, N=1, dx_scale=1.):
    ''' G = dy (y > 0 if relu) (row valid); dx = scale G W (zero on masked rows), dw = G^T x, db = sum_m G; a*: sums of |addends| '''
    x = d(x).reshape(-1, x.shape[-1])
    M = x.shape[0]
    g = d(dy).reshape(M, -1).copy()
    if relu:
        g *= (d(y).reshape(M, -1) > 0)
    if mask_lengths is not None:
        g *= row_mask(mask_lengths, M // N, N).reshape(-1, 1)
    s = f32(dx_scale)
    # linear_rows_bwd_dw_kernel walks the rows in order (cw, cb: the bounds of those chains); the generic kernel does not
    cw = chain_bound(g.T[:, None, :] * x.T[None]) if ls_few_rows(M, mask_lengths is not None) else None
    cb = chain_bound(g.T) if cw is not None else None
    return LsBwd(s * (g @ d(w)), abs(s) * (np.abs(g) @ np.abs(d(w))), g.T @ x, np.abs(g).T @ np.abs(x), g.sum(0), np.abs(g).sum(0), cw, cb)


def rows_dw_bound(chain, con, old):
    ''' linear_rows_bwd_dw_kernel: the chain over the rows, then one atomic onto the old value '''
    return chain + gamma(1) * (np.abs(d(old)) + np.abs(con) + chain)


def colsum(x):
    x = d(x).reshape(-1, x.shape[-1])
    return x.sum(0), np.abs(x).sum(0)


# ---------------------------------------------------------------------------------------------------- FiLM head
FilmHead = namedtuple('FilmHead', 'z32 g_raw b_raw eg eb films efilms')


def film_head_fwd(emb, spk_table, ids, wg, bg, wb, bb, post, nb, ch):
    ''' z = emb + spk_table[id] (fp32, one rounding: the projections see the ROUNDED z); g_raw = z Wg^T + bg, b_raw = z Wb^T + bb;
        films as film_assemble_fwd, with the error of the raw values carried through '''
    z32 = gather_add_fwd32(emb, spk_table, ids)
    g_raw, eg = dense(z32, wg, bg)
    b_raw, eb = dense(z32, wb, bb)
    films, efilms = film_assemble_fwd(g_raw, b_raw, post, nb, ch, eg, eb)
    return FilmHead(z32, g_raw, b_raw, eg, eb, films, efilms)


FilmHeadBwd = namedtuple('FilmHeadBwd', 'd_emb a_emb d_spk a_spk share dpost apost dwg awg dbg abg dwb awb dbb abb e_chain t_abs')


def film_head_bwd(g_raw, b_raw, post, z, ids, wg, wb, dfilms, nb, ch, n_spk):
    ''' every gradient of dx_film_head_bwd as a contribution: dz = dg_raw Wg + db_raw Wb goes to d_emb[b] and to d_spk[ids[b]];
        dWg = dg_raw^T z, dbg = sum_b dg_raw, the same for the betas; dpost as film_assemble_bwd.  share: utterances per speaker row '''
    r = film_assemble_bwd(g_raw, b_raw, post, dfilms, nb, ch)
    dz = r.dg_raw @ d(wg) + r.db_raw @ d(wb)
    az = np.abs(r.dg_raw) @ np.abs(d(wg)) + np.abs(r.db_raw) @ np.abs(d(wb))
    d_spk, a_spk, share = scatter_rows(ids, dz, n_spk)
    a_spk = scatter_rows(ids, az, n_spk)[0]
    zz = d(z)
    # film_head_bwd_dx_kernel: a workgroup owns 128 columns and walks them in order, gamma and beta interleaved -- a chain in a known
    # order (e_chain: its bound, summed over the workgroups) -- and the workgroups' sums t meet in atomics (t_abs: sum of |t| + bound)
    W = r.dg_raw.shape[1]
    e_chain, t_abs = np.zeros_like(dz), np.zeros_like(dz)
    for c0 in range(0, W, 128):
        c1 = min(W, c0 + 128)
        P = np.stack([r.dg_raw[:, None, c0:c1] * d(wg)[c0:c1].T[None], r.db_raw[:, None, c0:c1] * d(wb)[c0:c1].T[None]], axis=-1)
        P = P.reshape(P.shape[0], P.shape[1], -1)
        e = chain_bound(P)
        e_chain += e
        t_abs += np.abs(P.sum(-1)) + e
    return FilmHeadBwd(dz, az, d_spk, a_spk, share, r.dpost, r.apost,
                       r.dg_raw.T @ zz, np.abs(r.dg_raw).T @ np.abs(zz), r.dg_raw.sum(0), np.abs(r.dg_raw).sum(0),
                       r.db_raw.T @ zz, np.abs(r.db_raw).T @ np.abs(zz), r.db_raw.sum(0), np.abs(r.db_raw).sum(0), e_chain, t_abs)


def head_dx_bounds(bw, ids, W, old_emb, old_spk):
    ''' (bound of d_emb, bound of d_spk_table): the chains, then ceil(W / 128) atomics per utterance landing on the address '''
    nwg = cdiv(W, 128)
    e_emb = bw.e_chain + gamma(nwg) * (np.abs(d(old_emb)) + bw.t_abs)
    n_spk = old_spk.shape[0]
    e_spk = scatter_rows(ids, bw.e_chain, n_spk)[0] + gamma(nwg * np.maximum(bw.share, 1))[:, None] * (np.abs(d(old_spk)) + scatter_rows(ids, bw.t_abs, n_spk)[0])
    return e_emb, e_spk


# ---------------------------------------------------------------------------------------------------- speaker classifier
Classifier = namedtuple('Classifier', 'h1 e1 h2 e2 logits e3')


def classifier_fwd(emb, w1, b1, w2, b2, w3, b3, h1_in=None, h2_in=None):
    ''' gradient reversal (identity forward) -> Linear, ReLU, Linear, ReLU, Linear.  h1_in / h2_in: the fp32 values the next layer was
        actually fed (the kernel's own outputs); without them the layers chain and the bounds propagate '''
    h1, e1 = dense(emb, w1, b1, relu=True)
    h2, e2 = dense(h1 if h1_in is None else h1_in, w2, b2, relu=True, ex=e1 if h1_in is None else 0.)
    lg, e3 = dense(h2 if h2_in is None else h2_in, w3, b3, ex=e2 if h2_in is None else 0.)
    return Classifier(h1, e1, h2, e2, lg, e3)


ClassifierBwd = namedtuple('ClassifierBwd', 'd_emb e_emb g1 g2 dw adw db adb')


def classifier_bwd(d_logits, emb, h1, h2, w1, w2, w3, lam):
    ''' g3 = d_logits, g2 = (g3 W3) (h2 > 0), g1 = (g2 W2) (h1 > 0), d_emb = -lambda (g1 W1); dW_i = g_i^T input_i, db_i = sum_b g_i.
        d_emb is WRITTEN (e_emb its bound); dw / db are contributions, and adw / adb already hold the part of the bound that comes
        from the rounded g1 / g2 (as an absolute term to add to acc_bound) in the second element of each pair '''
    g3, S = d(d_logits), d_logits.shape[1]
    w1, w2, w3 = d(w1), d(w2), d(w3)
    gate2, gate1 = d(h2) > 0, d(h1) > 0
    chain = lambda g, w: chain_bound(g[:, None, :] * w.T[None])        # o ascending for every (b, k): a chain in a known order
    g2 = (g3 @ w3) * gate2
    e2 = chain(g3, w3) * gate2
    g1 = (g2 @ w2) * gate1
    e1 = (chain(g2, w2) + e2 @ np.abs(w2)) * gate1
    lam32 = f32(lam)
    d_emb = -lam32 * (g1 @ w1)
    e_emb = abs(lam32) * (chain(g1, w1) + e1 @ np.abs(w1)) + U32 * np.abs(d_emb)
    xs = (d(emb), d(h1), d(h2))
    gs, es = (g1, g2, g3), (e1, e2, 0. * g3)
    dw = [g.T @ x for g, x in zip(gs, xs)]
    adw = [(np.abs(g).T @ np.abs(x), e.T @ np.abs(x)) for g, e, x in zip(gs, es, xs)]
    db = [g.sum(0) for g in gs]
    adb = [(np.abs(g).sum(0), e.sum(0)) for g, e in zip(gs, es)]
    return ClassifierBwd(d_emb, e_emb, g1, g2, dw, adw, db, adb)


# ---------------------------------------------------------------------------------------------------- cases
MODEL_LAYOUT = ((4, 1, 4), (128, 256, 128))        # (nb, ch) as model.film_layout builds them from the default hparams
ODD_LAYOUT = ((2, 1, 3), (48, 80, 128))            # waves span blocks; W = 560 is no multiple of 64, 128 or 256

SE_FWD_SHAPES = {(3, 7): [7, 4, 0], (1, 1): [1], (3, 70): [70, 33, 0]}
SE_BWD_SHAPES = [(2, 70), (2, 64), (1, 1), (100, 300)]
SE_BWD_BIG = (257, 1025)
EMBED_SHAPES = {(3, 7): [7, 0, 4], (2, 70): [70, 33]}
MEAN_N = (1, 7, 8, 9, 70)
LS_MASKED = {(4, 7, 256, 3): [7, 0, 3, 1], (5, 33, 128, 1): [20, 33, 0, 30, 32], (5, 33, 128, 17): [20, 33, 0, 30, 32]}
LS_PLAIN = [(513, 128, 5), (512, 132, 70)]
TRANSPOSE_SHAPES = [(2, 1, 1), (1, 33, 31), (3, 80, 70), (2, 32, 64)]
COLSUM_ROWS, COLSUM_C = (1, 64, 65, 700), (1, 128, 300)
FILL_OFFSETS, FILL_COUNTS = tuple(range(17)), (0, 1, 15, 16, 17, 31, 4096 + 5, 2 * 4096 + 21)
HEAD_B = (1, 2, 5)
CLS_B, CLS_S = (1, 5), (1, 10, 127, 128)


def se_lengths(B, N, kind):
    ''' the length vectors every scalar_embed_bwd shape runs with '''
    if kind == 'none':
        return None
    if kind == 'full':
        return [N] * B
    if kind == 'zero':
        return [0] * B
    out = [N, max(N // 2 - 2, 0), 0, 1, N - 1] * cdiv(B, 5)          # ragged: full, about half, 0, 1, one short
    return out[:B]


def se_impulses(B, N):
    ''' [(b, n of the dout row, n of the only non-zero feature row, what)] for one utterance b = B - 1: first and last row of every
        slab with the feature only in the row before / behind it (the halo), rows 0 and N - 1 (zero padding: no tap reaches a
        neighbour outside), and the row itself '''
    b, out = B - 1, []
    for n0, n1 in se_slabs(B, N):
        for n, j, what in ((n0, n0 - 1, 'slab first, halo before'), (n1 - 1, n1, 'slab last, halo behind'), (n0, n0, 'slab first, centre')):
            if 0 <= j < N:
                out.append((b, n, j, what))
    out.append((b, 0, min(1, N - 1), 'row 0'))
    out.append((b, N - 1, max(N - 2, 0), 'row N - 1'))
    return out
