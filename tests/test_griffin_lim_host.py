"""Griffin-Lim preview path, CPU side: the float64 restatement (tests/griffin_lim_oracle.py) against what the REFERENCE's
`griffin_lim.py` produced (tests/golden/griffin_lim.npz, tools/gen_golden_griffin_lim.py), the new C-ABI entry points'
argument checks, and the WAV writer."""
import os
import struct

import numpy as np
import pytest

from tests import griffin_lim_oracle as O
from tests.util import make_hparams

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'griffin_lim.npz')
GL_T = (3, 24, 64, 100)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize('T', GL_T)
def test_oracle_matches_reference_fixture(T):
    fx = np.load(GOLD)
    hp = make_hparams()
    n_fft, hop = hp.filter_length, hp.hop_length
    mag = O.harmonic_magnitude(T)[:, :-2]
    S = O.n_samples(T, n_fft, hop)
    sig30 = fx[f'gl_{T}_sig30']
    assert sig30.shape == (S,) and S == (T - 2) * hop + n_fft and O.n_frames(T) == T - 2
    x0 = O.reference_start(int(fx[f'gl_{T}_seed']), S)
    sigs, proposal = O.griffin_lim(mag, hop, 30, x0)
    assert proposal.shape == (T - 2, n_fft // 2 + 1)
    if f'gl_{T}_sig1' in fx.files:
        assert _rel(sigs[0], fx[f'gl_{T}_sig1']) <= 1e-6
    assert _rel(sigs[29], sig30) <= 1e-6
    assert np.abs(sigs[29][-hop:]).max() == 0.             # the trailing hop of zeros
    if f'gl_{T}_norm30' in fx.files:
        norm = O.normalise(sigs[29])
        assert np.abs(norm - fx[f'gl_{T}_norm30']).max() <= 1e-6 and np.abs(norm).max() == 1.


def test_oracle_lengths_and_degenerate_cases():
    hp = make_hparams()
    assert [O.n_samples(T, 1024, 256) for T in (0, 1, 2, 3, 24)] == [1024, 1024, 1024, 1280, 6656]
    assert np.array_equal(O.normalise(np.zeros(1024)), np.zeros(1024))      # the reference: 0 / 0 = NaN
    assert O.filterbank(hp).shape == (hp.n_mel_channels, hp.filter_length // 2 + 1)


def test_filterbank_bins_lie_in_at_most_two_filters():
    ''' the sparse A^T r of dx_mel_to_linear relies on it (Slaney triangles between consecutive centre frequencies) '''
    for n_fft in (256, 1024, 4096):
        fb = O.filterbank(make_hparams(filter_length=n_fft, hop_length=n_fft // 4))
        assert (fb > 0).sum(0).max() <= 2
        nz = fb > 0
        for m in range(fb.shape[0]):                    # each filter one contiguous range (empty at n_fft 256: lo = hi)
            idx = np.nonzero(nz[m])[0]
            assert len(idx) == 0 or idx[-1] - idx[0] + 1 == len(idx)


def test_reference_nnls_restatement_matches_fixture():
    ''' the reference's own residuals are reproduced by the restated L-BFGS-B NNLS (needs scipy) and the whole reference
        pipeline by nnls + griffin_lim + normalise '''
    pytest.importorskip('scipy.optimize')
    fx = np.load(GOLD)
    hp = make_hparams()
    A = O.filterbank(hp)
    for name in ('cone', 'edge'):
        b = np.exp(fx[f'nnls_{name}_mel'])
        res = O.rel_residual(A, O.nnls_lbfgs(A, b), b)
        assert np.allclose(res, fx[f'nnls_{name}_relres'], rtol=1e-3, atol=1e-7)
    mel = fx['pipe_mel']
    lin = O.nnls_lbfgs(A, np.exp(mel))
    x0 = O.reference_start(int(fx['pipe_seed']), O.n_samples(mel.shape[1], hp.filter_length, hp.hop_length))
    sig = O.griffin_lim(lin[:, :-2], hp.hop_length, 30, x0)[0][-1]
    assert np.abs(O.normalise(sig) - fx['pipe_wav']).max() <= 1e-5


def test_new_symbols_exported_and_argument_errors_reported():
    from daft_exprt import _hip as H
    if not os.path.exists(H.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = H.lib()
    for name in ('dx_gl_tables', 'dx_mel_to_linear', 'dx_gl_ws_floats', 'dx_griffin_lim', 'dx_gl_noise', 'dx_gl_normalise'):
        assert hasattr(lib, name) and name in {p[0] for p in H.header_prototypes()}
    assert lib.dx_abi_version() == 13
    assert lib.dx_gl_ws_floats(4, 10, 1024) == 4 * 8 * 1024 and lib.dx_gl_ws_floats(4, 2, 1024) == 0
    P = 8                                                                    # a non-null pointer never dereferenced
    assert lib.dx_gl_tables(None, P, 1024, None) == -1 and b'null' in lib.dx_last_error()
    assert lib.dx_gl_tables(P, P, 512, None) == -5 and b'512' in lib.dx_last_error()
    args = [P] * 9 + [513 * 10, 1, 513, 2, 10, 80, 1024, 500, 1e-3, 1, None]
    assert lib.dx_mel_to_linear(*([None] + args[1:])) == -1 and b'null' in lib.dx_last_error()
    bad = list(args); bad[15] = 2048
    assert lib.dx_mel_to_linear(*bad) == -5 and b'n_fft=2048' in lib.dx_last_error()
    bad = list(args); bad[14] = 300
    assert lib.dx_mel_to_linear(*bad) == -2 and b'n_mel=300' in lib.dx_last_error()
    S = 8 * 256 + 1024
    gl = [P, 10 * 513, 1, 513, P, None, 0, P, P, P, S, P, P, 2, 10, 1024, 256, 30, 0, None]
    bad = list(gl); bad[0] = None
    assert lib.dx_griffin_lim(*bad) == -1 and b'null' in lib.dx_last_error()
    bad = list(gl); bad[16] = 300                                            # n_fft not a multiple of hop
    assert lib.dx_griffin_lim(*bad) == -5 and b'hop=300' in lib.dx_last_error()
    bad = list(gl); bad[15] = 2048
    assert lib.dx_griffin_lim(*bad) == -5 and b'n_fft=2048' in lib.dx_last_error()
    bad = list(gl); bad[10] = S - 1
    assert lib.dx_griffin_lim(*bad) == -2 and b'samples' in lib.dx_last_error()
    bad = list(gl); bad[17] = 0
    assert lib.dx_griffin_lim(*bad) == -2 and b'iters=0' in lib.dx_last_error()
    assert lib.dx_gl_noise(None, S, P, 2, 10, 1024, 256, 0, None) == -1
    assert lib.dx_gl_noise(P, S, P, 2, 10, 1000, 250, 0, None) == -5
    assert lib.dx_gl_normalise(None, S, P, 2, 10, 1024, 256, None) == -1
    assert lib.dx_gl_normalise(P, S, P, 2, 10, 1024, 100, None) == -5 and b'hop=100' in lib.dx_last_error()


def test_wav_writer_header_and_roundtrip(tmp_path):
    from daft_exprt.griffin_lim import write_wav
    x = np.sin(np.arange(1000) / 7.) * np.linspace(0, 1, 1000)
    path = str(tmp_path / 'a.wav')
    write_wav(path, 22050, x.astype(np.float32))
    raw = open(path, 'rb').read()
    assert raw[:4] == b'RIFF' and raw[8:12] == b'WAVE' and struct.unpack('<I', raw[4:8])[0] == len(raw) - 8
    assert raw[12:16] == b'fmt ' and struct.unpack('<I', raw[16:20])[0] == 18
    fmt, ch, rate, byte_rate, align, bits = struct.unpack('<HHIIHH', raw[20:36])
    assert (fmt, ch, rate, byte_rate, align, bits) == (3, 1, 22050, 22050 * 8, 8, 64)
    i = raw.index(b'data')
    assert struct.unpack('<I', raw[i + 4:i + 8])[0] == 8 * 1000 and len(raw) == i + 8 + 8000
    assert np.array_equal(np.frombuffer(raw[i + 8:], dtype='<f8'), x.astype(np.float32).astype(np.float64))
    try:
        from scipy.io import wavfile
    except ImportError:
        return
    sr, y = wavfile.read(path)
    assert sr == 22050 and y.dtype == np.float64 and np.array_equal(y, x.astype(np.float32).astype(np.float64))
