'''
GPU tests of the wavdir dataset (run with -m gpu): the ragged-batch STFT kernel of libdanet_prep_hip.so
against the reference's own golden vectors, the float64 restatement (tests/prep_ref.py) and the shipped
danet_stft path, its zero padding, guarded pitched output and bit-exact crop, the dataset end to end and
the command line.  BAR: 1e-5 of the utterance's maximum, the bar test_stft_against_reference_golden uses.
'''
import io
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import prep_ref as P
from gpu_helpers import check_lstm_status, cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'frontend_ref.npz')
BAR = 1e-5


def _window(N):
    import scipy.signal.windows
    return np.sqrt(scipy.signal.windows.hann(N)).astype(np.float32)


def _pool(waves, order=None):
    '''waveforms laid back to back in `order` -> (pool, offsets, lengths) indexed by utterance'''
    order = list(range(len(waves))) if order is None else order
    offs, off = [0] * len(waves), 0
    for u in order:
        offs[u] = off
        off += len(waves[u])
    pool = np.zeros(off, np.float32)
    for u in order:
        pool[offs[u]:offs[u] + len(waves[u])] = waves[u]
    return pool, offs, [len(w) for w in waves]


def _run(waves, pads, T_out, N, S, order=None, **kw):
    from danet_amd import ops
    pool, offs, lens = _pool(waves, order)
    desc = ops.prep_desc(offs, lens, pads, T_out, len(pool), N, S)
    return ops.stft_batch(cu(pool), desc, T_out, cu(_window(N)), N, S, **kw)


def _check_against(X, ref, frames, pads, what=''):
    '''each utterance's own frames within BAR of its maximum; every padding frame bitwise zero'''
    X = np.asarray(X)
    worst = 0.
    for u, (T, p) in enumerate(zip(frames, pads)):
        own, want = X[u, p:p + T].astype(np.complex128), ref[u, p:p + T]
        err = np.abs(own - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err < BAR, (what, u, err)
        assert not P.bits(X[u, :p]).any() and not P.bits(X[u, p + T:]).any(), (what, u)
    return worst


def test_golden_vectors_in_one_ragged_launch():
    g = np.load(GOLD)
    w256 = _window(256)
    assert np.array_equal(w256.view(np.uint32), g['wnd256_bits'])
    Ls = (256, 257, 319, 320, 8000, 8001, 8063, 8064)
    waves = [np.random.RandomState(0).randn(L).astype(np.float32) for L in Ls] + [g['stft256_int16scale_x']]
    gold = [g['stft256_L%d' % L] for L in Ls] + [g['stft256_int16scale']]
    frames = [len(x) for x in gold]
    for L, T in zip(Ls, frames):
        assert T == 1 + -(-L // 64)                                    # frame counts are exact
    T_out = max(frames) + 3
    order = [4, 0, 8, 2, 7, 1, 5, 3, 6]                                # shuffled pool order
    pads = [(7 * u + 1) % (T_out - T + 1) for u, T in enumerate(frames)]
    pads[0], pads[1], pads[3] = 5, 6, 9
    assert len(set(pads)) == len(pads)                                 # distinct pad_left values
    X = _run(waves, pads, T_out, 256, 64, order=order).cpu().numpy()
    assert X.shape == (9, T_out, 129) and X.dtype == np.complex64
    for u, (T, p) in enumerate(zip(frames, pads)):
        own = X[u, p:p + T]
        assert own.shape == gold[u].shape
        err = np.abs(own.astype(np.complex128) - gold[u]).max() / np.abs(gold[u]).max()
        print('golden utterance %d (L = %d): %.3g' % (u, len(waves[u]), err))
        assert err < BAR, (u, err)
        assert not P.bits(X[u, :p]).any() and not P.bits(X[u, p + T:]).any()     # padding: bitwise +0.0


def test_golden_512_long_utterance():
    g = np.load(GOLD)
    w = _window(512)
    assert np.array_equal(w.view(np.uint32), g['wnd512_bits'])
    x = np.random.RandomState(0).randn(160000).astype(np.float32)
    Xn = _run([x], [0], 1251, 512, 128).cpu().numpy()[0]
    assert Xn.shape == tuple(g['stft512_L160000_shape']) == (1251, 257)
    scale = np.abs(Xn).max()
    assert np.abs(Xn[:2] - g['stft512_L160000_head']).max() / scale < 1e-5
    assert np.abs(Xn[-2:] - g['stft512_L160000_tail']).max() / scale < 1e-5
    assert np.abs(Xn[600:602] - g['stft512_L160000_mid']).max() / scale < 1e-5
    assert abs(np.abs(Xn.astype(np.complex128)).sum() - g['stft512_L160000_abs_sum']) \
        < 1e-5 * g['stft512_L160000_abs_sum']


def _ragged(seed, n_utt, N, S, scale=1.0):
    rng = np.random.RandomState(seed)
    lens = [N] + [int(rng.randint(N, N + 6 * S + 1)) for _ in range(n_utt - 1)]
    waves = [(rng.randn(L) * scale).astype(np.float32) for L in lens]
    frames = [P.num_frames(L, N, S) for L in lens]
    T_out = max(frames) + 2
    pads = [int(rng.randint(0, T_out - T + 1)) for T in frames]
    return waves, frames, pads, T_out


def test_guarded_pitched_output_is_left_alone():
    from danet_amd import ops
    N, S = 256, 64
    waves, frames, pads, T_out = _ragged(5, 5, N, S, 1000.)
    F, ld, guard = N // 2 + 1, N // 2 + 1 + 3, 64
    n = len(waves)
    words = torch.full((2 * (guard + n * T_out * ld + guard),), 0x7fc00abc, dtype=torch.int32, device='cuda')
    flat = torch.view_as_complex(words.view(torch.float32).view(-1, 2))       # a NaN pattern everywhere
    before = flat.clone()
    out = flat[guard:guard + n * T_out * ld].view(n, T_out, ld)[:, :, :F]
    pool, offs, lens = _pool(waves)
    desc = ops.prep_desc(offs, lens, pads, T_out, len(pool), N, S)
    got = ops.stft_batch(cu(pool), desc, T_out, cu(_window(N)), N, S, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    a, b = P.bits(flat.cpu().numpy()), P.bits(before.cpu().numpy())
    assert np.array_equal(a[:2 * guard], b[:2 * guard]) and np.array_equal(a[-2 * guard:], b[-2 * guard:])
    body_a = a[2 * guard:-2 * guard].reshape(n, T_out, ld, 2)
    body_b = b[2 * guard:-2 * guard].reshape(n, T_out, ld, 2)
    assert np.array_equal(body_a[:, :, F:], body_b[:, :, F:])           # pitch gaps bit-unchanged
    assert not (body_a[:, :, :F] == 0x7fc00abc).any()                    # every element inside F written
    ref = P.batch_ref(waves, pads, T_out, _window(N), N, S)
    _check_against(out.cpu().numpy(), ref, frames, pads, 'pitched')
    dense = _run(waves, pads, T_out, N, S).cpu().numpy()
    assert np.array_equal(P.bits(dense), P.bits(out.cpu().numpy()))     # the pitch does not change a value


def test_agrees_with_the_shipped_stft_path():
    from danet_amd import ops
    for N, S in ((256, 64), (512, 128)):
        waves, frames, pads, T_out = _ragged(6, 7, N, S, 2000.)
        X = _run(waves, pads, T_out, N, S).cpu().numpy()
        w = cu(_window(N))
        for u, (x, T, p) in enumerate(zip(waves, frames, pads)):
            ref = ops.stft(cu(x), w, N, S).cpu().numpy()
            assert ref.shape == (T, N // 2 + 1)
            placed = np.zeros((T_out, N // 2 + 1), np.complex64)
            placed[p:p + T] = ref
            err = np.abs(X[u].astype(np.complex128) - placed).max() / np.abs(ref).max()
            assert err < BAR, (N, u, err)


def test_crop_equals_the_slice_of_the_full_launch_bit_for_bit():
    N, S = 256, 64
    rng = np.random.RandomState(8)
    lens = [256, 3000, 1111, 2048, 5000, 777]
    waves = [(rng.randn(L) * 3000).astype(np.float32) for L in lens]
    frames = [P.num_frames(L, N, S) for L in lens]
    T_out = max(frames) + 9
    pads = [9, 0, 30, 4, 5, 60]
    full = _run(waves, pads, T_out, N, S).cpu().numpy()
    windows = [(0, T_out), (0, 1), (T_out - 1, 1), (0, 4), (3, 8), (7, 13), (1, 64), (T_out - 5, 5),
               (T_out - 3, 3),            # wholly in padding for every utterance but the longest
               (2, 5), (8, 2), (20, 33), (59, 17), (5, T_out - 5)]
    for beg, cnt in windows:
        part = _run(waves, pads, T_out, N, S, t_begin=beg, t_count=cnt).cpu().numpy()
        assert part.shape == (len(waves), cnt, 129)
        assert np.array_equal(P.bits(part), P.bits(full[:, beg:beg + cnt])), (beg, cnt)
    # and n_utt does not change a value either
    one = _run(waves[2:3], pads[2:3], T_out, N, S).cpu().numpy()
    assert np.array_equal(P.bits(one[0]), P.bits(full[2]))


ENVELOPE = [(N, S) for N in (64, 256, 512, 4096) for S in (N // 4, N // 2, N)] + [(256, 48)]


@pytest.mark.parametrize('n_utt', [1, 2, 130])
@pytest.mark.parametrize('N,S', ENVELOPE)
def test_envelope_against_float64(N, S, n_utt):
    waves, frames, pads, T_out = _ragged(N + S + n_utt, n_utt, N, S, 500.)
    assert len(waves[0]) == N                                            # len_u = N exactly
    ref = P.batch_ref(waves, pads, T_out, _window(N), N, S)
    X = _run(waves, pads, T_out, N, S).cpu().numpy()
    worst = _check_against(X, ref, frames, pads, (N, S, n_utt))
    print('N %d S %d n_utt %d: worst %.3g' % (N, S, n_utt, worst))
    beg, cnt = T_out // 3, max(1, T_out // 2)
    part = _run(waves, pads, T_out, N, S, t_begin=beg, t_count=cnt).cpu().numpy()
    assert np.array_equal(P.bits(part), P.bits(X[:, beg:beg + cnt]))


@pytest.mark.parametrize('N,S', ENVELOPE)
def test_every_residue_of_the_length(N, S):
    rng = np.random.RandomState(N * 3 + S)
    for r0 in range(0, S, 128):
        lens = [N + r for r in range(r0, min(S, r0 + 128))]             # every residue of len mod S
        waves = [(rng.randn(L) * 500).astype(np.float32) for L in lens]
        frames = [P.num_frames(L, N, S) for L in lens]
        T_out = max(frames) + 1
        pads = [int(rng.randint(0, T_out - T + 1)) for T in frames]
        ref = P.batch_ref(waves, pads, T_out, _window(N), N, S)
        X = _run(waves, pads, T_out, N, S).cpu().numpy()
        _check_against(X, ref, frames, pads, (N, S, r0))


def test_descriptor_beyond_t_out_is_rejected_before_any_launch(monkeypatch):
    from danet_amd import _lib, ops
    lib = _lib.load_prep()
    calls = []
    real = lib.danet_prep_stft_batch

    class Spy(object):
        def __getattr__(self, name):
            if name == 'danet_prep_stft_batch':
                return lambda *a: calls.append(a) or real(*a)
            return getattr(lib, name)
    monkeypatch.setattr(_lib, '_prep', Spy())
    x = np.random.RandomState(1).randn(1000).astype(np.float32)
    T = P.num_frames(1000, 256, 64)
    bad = np.zeros(1, ops.PREP_DESC_DTYPE)
    bad[0] = (0, 1000, 2, 0)
    with pytest.raises(ValueError, match='exceeds T_out'):
        ops.stft_batch(cu(x), bad, T + 1, cu(_window(256)), 256, 64)
    bad[0] = (0, 200, 0, 0)
    with pytest.raises(ValueError, match='longer than input'):
        ops.stft_batch(cu(x), bad, T, cu(_window(256)), 256, 64)
    assert calls == []
    bad[0] = (0, 1000, 1, 0)
    ops.stft_batch(cu(x), bad, T + 1, cu(_window(256)), 256, 64)
    assert len(calls) == 1


def test_plan_is_cached_per_device_size_and_window():
    from danet_amd import ops
    x = np.random.RandomState(1).randn(3000).astype(np.float32)
    w = cu(_window(256))
    _run([x], [0], P.num_frames(3000, 256, 64), 256, 64)
    n0 = len(ops._prep_plans)
    a = ops._prep_plan(w, 256)
    assert ops._prep_plan(w, 256) is a and ops._prep_plan(cu(_window(256)), 256) is a
    assert len(ops._prep_plans) == n0
    assert ops._prep_plan(cu(np.ones(256, np.float32)), 256) is not a
    assert ops._prep_plan(cu(_window(512)), 512) is not a


# ------------------------------------------------------------------------- dataset end to end
def _tree_config(hp, root, **kw):
    base = dict(DATASET_TYPE='wavdir', DATASET_DIR=str(root), FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000,
                BATCH_SIZE=4, MAX_N_SIGNAL=2, MAX_TRAIN_LEN=64)
    base.update(kw)
    hp.load(base)
    hp.digest()


def test_dataset_device_route_equals_host_route_bit_for_bit(hp, tmp_path):
    from danet_amd import datasets, feed
    made = P.write_tree(tmp_path / 'tree', seed=3, n_per_subset=40)
    _tree_config(hp, tmp_path / 'tree')
    ds = datasets.WavDirData()
    ds.install_and_load()
    assert [len(ds.files[s]) for s in ('train', 'valid', 'test')] == [40, 40, 40]
    assert ds.files['train'] == sorted(made['train'])
    bs = hp.BATCH_SIZE * hp.MAX_N_SIGNAL
    window = _window(256)

    def device_run():
        random.seed(21)
        np.random.seed(22)
        return [b.cpu().numpy().copy() for _ in range(2)
                for b in ds.epoch_device('train', bs, shuffle=True, device='cuda', crop_len=hp.MAX_TRAIN_LEN)]

    dev = device_run()
    random.seed(21)
    np.random.seed(22)
    host = [np.ascontiguousarray(feed.to_batch_host(pt, hp.MAX_TRAIN_LEN)) for _ in range(2)
            for pt in ds.epoch('train', bs, shuffle=True)]
    assert len(dev) == len(host) == 2 * 5
    for a, b in zip(dev, host):
        assert a.shape == b.shape == (hp.BATCH_SIZE, hp.MAX_N_SIGNAL, hp.MAX_TRAIN_LEN, hp.FEATURE_SIZE)
        assert a.dtype == b.dtype == np.complex64
        assert np.array_equal(P.bits(a), P.bits(b))
    again = device_run()
    for a, b in zip(dev, again):
        assert np.array_equal(P.bits(a), P.bits(b))
    # against the restatement: same plan, same draws, float64 scipy
    random.seed(21)
    np.random.seed(22)
    k = 0
    for _ in range(2):
        for idx in P.index_plan(40, bs, True):
            waves = [ds.pool_host['train'][ds.offsets['train'][i]:ds.offsets['train'][i] + ds.lengths['train'][i]]
                     for i in idx]
            T_max, pads = P.draw_pads([P.num_frames(len(w), 256, 64) for w in waves])
            beg, cnt = P.draw_crop(T_max, hp.MAX_TRAIN_LEN)
            ref = P.batch_ref(waves, pads, T_max, window, 256, 64, beg, cnt)
            got = dev[k].reshape(bs, cnt, -1).astype(np.complex128)
            for u in range(bs):
                full = np.abs(P.stft_ref(waves[u], window, 256, 64)).max()
                assert np.abs(got[u] - ref[u]).max() / full < BAR, (k, u)
            k += 1
    # validation: no crop, the whole padded batch
    random.seed(4)
    v = [b.cpu().numpy().copy() for b in ds.epoch_device('valid', bs, device='cuda')]
    random.seed(4)
    vh = [feed.to_batch_host(pt, None) for pt in ds.epoch('valid', bs)]
    assert len(v) == 5
    for a, b in zip(v, vh):
        assert np.array_equal(P.bits(a), P.bits(np.ascontiguousarray(b)))


def _small_model_cfg(root):
    return dict(BATCH_SIZE=4, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2,
                LSTM_HDIM=8, NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='anchor',
                INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE='dot-softmax-orig', MAX_TRAIN_LEN=64,
                DATASET_TYPE='wavdir', DATASET_DIR=str(root))


def test_train_epoch_fast_route_equals_sync_feed_bit_for_bit(hp, tmp_path):
    from danet_amd import cli, datasets, feed
    from danet_amd.model import Model
    P.write_tree(tmp_path / 'tree', seed=5, n_per_subset=24, subsets=('train', 'test'), seconds=(0.2, 0.5))

    def run(sync):
        hp.reset()
        hp.load(_small_model_cfg(tmp_path / 'tree'))
        hp.digest()
        ds = datasets.WavDirData()
        ds.load_host(out=io.StringIO())
        ds.is_loaded = True
        model = Model('loop', device='cuda', seed=5).build()
        random.seed(9)
        np.random.seed(10)
        out = io.StringIO()
        src = feed.EpochSource(ds, 'train', hp.BATCH_SIZE * hp.MAX_N_SIGNAL, shuffle=True)
        rep, n = cli.train_epoch(model, src, out, sync_feed=sync)
        vrep = cli.evaluate(model, ds, 'valid', out, sync_feed=sync)
        model.check_status()
        return rep, n, vrep, model._flat.detach().cpu().numpy().copy()

    rep_s, n_s, v_s, p_s = run(True)
    rep_a, n_a, v_a, p_a = run(False)
    check_lstm_status()
    assert n_s == n_a == 3
    assert list(rep_s) == list(rep_a) == ['loss', 'SNR', 'LR']
    for k in rep_s:
        assert np.isfinite(rep_s[k]) and rep_s[k] == rep_a[k], (k, rep_s[k], rep_a[k])      # bit for bit
    assert list(v_s) == list(v_a)
    for k in v_s:
        assert v_s[k] == v_a[k], (k, v_s[k], v_a[k])
    assert np.array_equal(p_s, p_a)


def test_command_line_train_valid_and_sync_feed(tmp_path):
    P.write_tree(tmp_path / 'tree', seed=6, n_per_subset=16, subsets=('train', 'test'), seconds=(0.2, 0.5))
    cfg = tmp_path / 'cfg.json'
    cfg.write_text(json.dumps(_small_model_cfg(tmp_path / 'tree')))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('DANET_FEED_MODE', None)

    def main(*args):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py')] + list(args), cwd=str(tmp_path),
                             capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        return out.stdout

    txt = main('-n', 'wd', '-m', 'train', '-ds', 'wavdir', '-c', str(cfg), '-ne', '1', '-bs', '4',
               '-o', str(tmp_path / 'final.npz'))
    assert 'wavdir train: 16 files' in txt and 'Epoch 1/1' in txt and 'Valid  1/1' in txt
    loss = float(txt.split('Epoch 1/1 loss=')[1].split()[0])
    assert np.isfinite(loss)
    assert (tmp_path / 'saves' / 'wd_e1.npz').exists() and (tmp_path / 'final.npz').exists()
    txt = main('-n', 'wd', '-m', 'valid', '-ds', 'wavdir', '-c', str(cfg), '-bs', '4',
               '-i', str(tmp_path / 'final.npz'))
    assert 'Valid: ' in txt and np.isfinite(float(txt.split('Valid: loss=')[1].split()[0]))
    txt2 = main('-n', 'wd2', '-m', 'train', '-ds', 'wavdir', '-c', str(cfg), '-ne', '1', '-bs', '4', '--sync-feed')
    assert np.isfinite(float(txt2.split('Epoch 1/1 loss=')[1].split()[0]))
    assert (tmp_path / 'saves' / 'wd2_e1.npz').exists()
