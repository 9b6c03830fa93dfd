'''
GPU tests of the online attractor estimator (libdanet_online_hip.so, include/danet_online_hip.h) against the float64
restatement of tests/online_ref.py.  Every output and the state lie between poisoned guard bands.

(a) single-frame scans (T = 1, a random state, arbitrary embeddings) over F x E x C x activation, every written value;
(b) trajectories of the case table (clustered embeddings) over T x B x lambda; (c) bit for bit: cuts, rows of a batch,
repeats, the hold, guard bands, argument errors; (d) danet_online_separate against float64 within the header's derived
bound, and against ops.SeparateFn; (e) Model.infer / valid_step / `main.py -m demo` with the "online" estimator.

The bar of (a) and (b) is 1e-5 of each output's maximum (online_ref.BAR), the bar this project holds its recurrent
kernels to; test_online_cpu.py shows that the float32 restatement alone stays within 1e-6 on the trajectory cases.
'''
import io
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import online_ref as OR
from gpu_helpers import ROOT, check_lstm_status

pytestmark = pytest.mark.gpu

POISON = -7.25e33
GUARD = 1024


def _guarded(shape, dtype=torch.float32, fill=None):
    '''(whole buffer, the view of `shape` in its middle): everything poisoned, or the middle set to `fill`'''
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device='cuda')
    view = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        view.copy_(torch.as_tensor(np.ascontiguousarray(fill)).to(dtype))
    return buf, view


def _intact(*bufs):
    return all(bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all()) for b in bufs)


def _cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _scan(V, W, state, act, lam, T0, eps=OR.EPS, t_first=0):
    '''one danet_online_scan from the numpy state (S, n, A) -> (attr float32 [B, T, C, E], the state after (S, n, A)
    float64), both read back; the guard bands around attr and state checked'''
    from danet_amd import ops
    B, T, F, E = V.shape
    C = state[2].shape[1]
    sbuf, st = _guarded((B, OR.state_doubles(C, E)), torch.float64, OR.pack(state))
    abuf, attr = _guarded((B, T, C, E))
    got = ops.online_scan(_cu(V), _cu(W), st, act, lam, T0, eps, t_first, attr=attr)
    assert got is attr
    torch.cuda.synchronize()
    assert _intact(sbuf, abuf)
    return attr.cpu().numpy(), OR.unpack(st.cpu().numpy(), C, E)


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ------------------------------------------------------------------------------------ (a) single frames
@pytest.mark.parametrize('E', OR.SHAPE_E)
@pytest.mark.parametrize('F', OR.SHAPE_F)
def test_single_frame_scan_against_float64(F, E):
    worst = 0.0
    for C in OR.SHAPE_C:
        for act in (0, 1):
            V, W, state = OR.random_case(2, 1, F, E, C, seed=F * 7 + E * 3 + C + act)
            lam = (1.0, 0.95, 0.5)[(C + act) % 3]
            attr, (S, n, A) = _scan(V, W, state, act, lam, 3, t_first=5)
            wattr, (wS, wn, wA) = OR.scan(V, W, state, act, lam, 3, OR.EPS, t_first=5)
            errs = [_rel(attr, wattr), _rel(S, wS), _rel(n, wn), _rel(A, wA)]
            worst = max(worst, *errs)
            assert max(errs) <= OR.BAR, (C, act, errs)
            assert np.array_equal(attr[:, 0].astype(np.float64), A)          # the state's A is the last attractor
            assert np.abs(attr[:, 0] - state[2]).max() > 1e-3                # and it moved
    print('single frame F %d E %d: worst error %.3g of the maximum' % (F, E, worst))


def test_single_frame_in_the_hold_accumulates_and_keeps_a0():
    V, W, state = OR.random_case(3, 1, 65, 20, 3, seed=1)
    attr, (S, n, A) = _scan(V, W, state, 0, 0.9, 8, t_first=7)
    wattr, (wS, wn, wA) = OR.scan(V, W, state, 0, 0.9, 8, OR.EPS, t_first=7)
    assert np.array_equal(A, state[2]) and np.array_equal(attr[:, 0].astype(np.float64), state[2])
    assert max(_rel(S, wS), _rel(n, wn)) <= OR.BAR and np.abs(S - state[0]).max() > 1e-3
    # eps above every n: nothing moves either, whatever t
    attr, (_, _, A) = _scan(V, W, state, 0, 0.9, 8, eps=1e30, t_first=100)
    assert np.array_equal(A, state[2]) and np.array_equal(attr[:, 0].astype(np.float64), state[2])


# ------------------------------------------------------------------------------------ (b) trajectories
_GRID = [(T, B, lam) for T in OR.TRAJECTORY_T for B in OR.TRAJECTORY_B for lam in OR.TRAJECTORY_LAMBDA]


@pytest.mark.parametrize('i', range(len(_GRID)))
def test_trajectory_against_float64(i):
    T, B, lam = _GRID[i]
    F, E, C, act = OR.TRAJECTORY_SHAPES[i % len(OR.TRAJECTORY_SHAPES)]
    V, W, A0 = OR.clustered_case(B, T, F, E, C, seed=i)
    from danet_amd import ops
    attr = ops.online_attractors(_cu(V), _cu(W), _cu(A0), act, lam, OR.T0, OR.EPS)
    assert tuple(attr.shape) == (B, T, C, E) and attr.dtype == torch.float32
    attr = attr.cpu().numpy()
    want = OR.attractors(V, W, A0, act, lam, OR.T0, OR.EPS)
    f32 = _rel(OR.attractors(V, W, A0, act, lam, OR.T0, OR.EPS, np.float32), want)
    err = _rel(attr, want)
    print('trajectory T %d B %d lambda %g F %d E %d C %d act %d: kernel %.3g, float32 restatement %.3g of max |A|'
          % (T, B, lam, F, E, C, act, err, f32))
    assert err <= OR.BAR
    # frames t < T0 carry A0
    hold = min(T, OR.T0)
    assert np.array_equal(attr[:, :hold], np.broadcast_to(A0[:, None], (B, hold, C, E)))
    if T > OR.T0:
        assert np.abs(attr[:, OR.T0:] - A0[:, None]).max() > 1e-2


# ------------------------------------------------------------------------------------ (c) bit for bit
@pytest.mark.parametrize('F,E,C,act,lam', [(129, 20, 2, 1, 0.95), (33, 7, 4, 0, 1.0), (300, 64, 3, 0, 0.5)])
def test_cut_scans_equal_the_whole_bit_for_bit(F, E, C, act, lam):
    B, T = 3, 70
    V, W, A0 = OR.clustered_case(B, T, F, E, C, seed=F)
    whole, end = _scan(V, W, OR.init(A0), act, lam, OR.T0)
    again, end_again = _scan(V, W, OR.init(A0), act, lam, OR.T0)
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))                  # repeated calls agree
    assert np.array_equal(OR.pack(end).view(np.uint64), OR.pack(end_again).view(np.uint64))
    for cut in (1, OR.T0 - 1, OR.T0, OR.T0 + 1, 35):
        a, mid = _scan(V[:, :cut], W[:, :cut], OR.init(A0), act, lam, OR.T0)
        b, end2 = _scan(V[:, cut:], W[:, cut:], mid, act, lam, OR.T0, t_first=cut)
        assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint32), whole.view(np.uint32)), cut
        assert np.array_equal(OR.pack(end2).view(np.uint64), OR.pack(end).view(np.uint64)), cut
    # three calls, and a block of one frame in the middle
    a, s1 = _scan(V[:, :9], W[:, :9], OR.init(A0), act, lam, OR.T0)
    b, s2 = _scan(V[:, 9:10], W[:, 9:10], s1, act, lam, OR.T0, t_first=9)
    c, s3 = _scan(V[:, 10:], W[:, 10:], s2, act, lam, OR.T0, t_first=10)
    assert np.array_equal(np.concatenate([a, b, c], axis=1).view(np.uint32), whole.view(np.uint32))
    assert np.array_equal(OR.pack(s3).view(np.uint64), OR.pack(end).view(np.uint64))


def test_a_row_alone_equals_the_row_inside_a_launch_of_33():
    B, T, F, E, C = 33, 20, 129, 20, 2
    V, W, A0 = OR.clustered_case(B, T, F, E, C, seed=33)
    whole, end = _scan(V, W, OR.init(A0), 0, 0.95, OR.T0)
    for b in (0, 7, 32):
        one, end1 = _scan(V[b:b + 1], W[b:b + 1], OR.init(A0[b:b + 1]), 0, 0.95, OR.T0)
        assert np.array_equal(one[0].view(np.uint32), whole[b].view(np.uint32)), b
        assert np.array_equal(OR.pack(end1)[0].view(np.uint64), OR.pack(end)[b].view(np.uint64)), b


def test_init_writes_the_layout_between_intact_guards():
    from danet_amd import ops
    B, C, E = 5, 3, 7
    A0 = np.random.RandomState(0).standard_normal((B, C, E)).astype(np.float32)
    sbuf, st = _guarded((B, OR.state_doubles(C, E)), torch.float64)
    assert ops.online_init(_cu(A0), st) is st
    torch.cuda.synchronize()
    assert _intact(sbuf)
    S, n, A = OR.unpack(st.cpu().numpy(), C, E)
    assert not S.any() and not n.any() and np.array_equal(A, A0.astype(np.float64))
    assert not np.signbit(S).any() and not np.signbit(n).any()
    fresh = ops.online_init(_cu(A0))
    assert fresh.dtype == torch.float64 and tuple(fresh.shape) == (B, ops.online_state_bytes(C, E) // 8)
    assert np.array_equal(fresh.cpu().numpy(), st.cpu().numpy())


def test_argument_errors_launch_nothing():
    from danet_amd import _lib, ops
    B, T, F, E, C = 2, 5, 33, 8, 2
    V, W, A0 = OR.clustered_case(B, T, F, E, C, seed=4)
    state = OR.pack(OR.init(A0))
    sbuf, st = _guarded(state.shape, torch.float64, state)
    abuf, attr = _guarded((B, T, C, E))
    obuf, out = _guarded((B, C, T, F))
    v, w = _cu(V), _cu(W)
    for kw in (dict(act=2), dict(lam=0.0), dict(lam=1.5), dict(T0=0), dict(t_first=-1), dict(eps=-1.0)):
        a = dict(dict(act=0, lam=0.9, T0=2, eps=OR.EPS, t_first=0), **kw)
        with pytest.raises(_lib.DanetHipError) as e:
            ops.online_scan(v, w, st, a['act'], a['lam'], a['T0'], a['eps'], a['t_first'], attr=attr)
        assert 'libdanet_online_hip error -1: scan: ' in str(e.value), kw
    with pytest.raises(_lib.DanetHipError):
        ops.online_separate(w, attr, v, 3, out=out)
    lib = _lib.load_online()
    assert lib.danet_online_scan(_lib.stream(), B, C, T, 1026, E, 0, 0.9, 2, 0, 1e-7, v.data_ptr(), w.data_ptr(),
                                 st.data_ptr(), attr.data_ptr()) == -1
    assert lib.danet_online_init(_lib.stream(), B, 5, E, _cu(A0).data_ptr(), st.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((abuf == POISON).all()) and bool((obuf == POISON).all()) and _intact(sbuf)
    assert np.array_equal(st.cpu().numpy(), state)


# ------------------------------------------------------------------------------------ (d) the separator
@pytest.mark.parametrize('E', OR.SHAPE_E)
@pytest.mark.parametrize('F', OR.SHAPE_F)
def test_separate_against_float64_within_the_derived_bound(F, E):
    from danet_amd import ops
    worst = 0.0
    for C in OR.SHAPE_C:
        for act in (0, 1):
            for T, B in ((1, 1), (5, 3)):
                rng = np.random.RandomState(F + 11 * E + C + act + T)
                V = rng.standard_normal((B, T, F, E)).astype(np.float32)
                W = (10 * np.abs(rng.standard_normal((B, T, F)))).astype(np.float32)
                attr = rng.standard_normal((B, T, C, E)).astype(np.float32)
                obuf, out = _guarded((B, C, T, F))
                assert ops.online_separate(_cu(W), _cu(attr), _cu(V), act, out=out) is out
                torch.cuda.synchronize()
                assert _intact(obuf)
                want = OR.separate(V, W, attr, act)
                bound = OR.separate_bound(V, W, attr)
                ratio = np.abs(out.cpu().numpy() - want) / bound
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1).all(), (C, act, T, B, float(ratio.max()))
    print('separate F %d E %d: worst error %.3g of the derived bound' % (F, E, worst))


@pytest.mark.parametrize('act', [0, 1])
def test_separate_with_a_repeated_attractor_set_agrees_with_the_separator(act):
    from danet_amd import ops
    B, T, F, E, C = 3, 6, 129, 20, 2
    rng = np.random.RandomState(act)
    V = rng.standard_normal((B, T, F, E)).astype(np.float32)
    W = (10 * np.abs(rng.standard_normal((B, T, F)))).astype(np.float32)
    one = rng.standard_normal((B, C, E)).astype(np.float32)
    attr = np.ascontiguousarray(np.broadcast_to(one[:, None], (B, T, C, E)))
    got = ops.online_separate(_cu(W), _cu(attr), _cu(V).view(B, T * F, E), act).cpu().numpy()
    plain, _ = ops.SeparateFn.apply(_cu(W), _cu(one), _cu(V).view(B, T * F, E), act, False)
    bound = OR.separate_bound(V, W, attr)
    assert got.shape == (B, C, T, F) == tuple(plain.shape)
    assert (np.abs(got - OR.separate(V, W, attr, act)) <= bound).all()
    ratio = np.abs(got.astype(np.float64) - plain.cpu().numpy()) / bound
    print('separate against ops.SeparateFn, act %d: worst difference %.3g of the derived bound' % (act, float(ratio.max())))
    assert (ratio <= 1).all()                                  # the same bar as against float64


# ------------------------------------------------------------------------------------ (e) the model
TINY = dict(BATCH_SIZE=2, MAX_N_SIGNAL=2, FFT_SIZE=64, FFT_STRIDE=16, EMBED_SIZE=4, NUM_LSTM_LAYERS=2, LSTM_HDIM=8,
            NUM_ANCHOR=4, ENCODER_TYPE='bilstm-orig', TRAIN_ESTIMATOR_METHOD='truth-weighted',
            SEPARATOR_TYPE='dot-softmax-orig')


def _model(hp, **keys):
    from danet_amd.model import Model
    hp.reset()
    hp.load(dict(TINY, **keys))
    hp.digest()
    return Model('online', device='cuda:0', seed=5).build()


def _signals(T, seed=0):
    rng = np.random.RandomState(seed)
    src = (rng.standard_normal((2, 2, T, 33)) + 1j * rng.standard_normal((2, 2, T, 33))).astype(np.complex64) * 3
    return _cu(src), _cu(src.sum(1))


def _bits(t):
    return torch.view_as_real(t).cpu().numpy().view(np.uint32)


def test_infer_within_the_hold_is_the_anchor_estimator_bit_for_bit(hp):
    from danet_amd import _lib
    src, mix = _signals(20)
    want = _bits(_model(hp, INFER_ESTIMATOR_METHOD='anchor').infer(mix))
    mapped = _lib._online is not None
    model = _model(hp, INFER_ESTIMATOR_METHOD='online')                    # T0 = 32 >= 20
    assert model.online == (32, 1.0)
    assert np.array_equal(_bits(model.infer(mix)), want)
    model = _model(hp, INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=20, ONLINE_MEMORY_FRAMES=10)
    assert np.array_equal(_bits(model.infer(mix)), want)
    assert (_lib._online is not None) == mapped                            # the hold path maps nothing
    check_lstm_status()


def test_a_model_with_another_estimator_never_maps_the_library():
    '''a fresh process builds a model with the `anchor` estimator, runs infer and valid_step, and ends with the library
    neither loaded nor mapped'''
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import __graft_entry__ as g; g.load_package()\n"
        "from danet_amd import _lib\n"
        "from danet_amd.hparams import hparams\n"
        "from danet_amd.model import Model\n"
        "hparams.load(%r); hparams.digest()\n"
        "model = Model('other', device='cuda:0', seed=5).build()\n"
        "rng = np.random.RandomState(0)\n"
        "src = torch.as_tensor((rng.standard_normal((2, 2, 40, 33)) + 1j * rng.standard_normal((2, 2, 40, 33)))"
        ".astype(np.complex64)).cuda()\n"
        "out = model.infer(src.sum(1)); res = model.valid_step(src); torch.cuda.synchronize()\n"
        "print('RAN:', tuple(out.shape) == (2, 2, 40, 33) and sorted(res) == ['SNR', 'loss'])\n"
        "print('STATE:', model.online)\n"
        "print('UNMAPPED:', _lib._online is None and 'libdanet_online' not in open('/proc/self/maps').read())\n"
        "print('CORE:', 'libdanet_hip' in open('/proc/self/maps').read())\n"
    ) % (ROOT, dict(TINY, INFER_ESTIMATOR_METHOD='anchor'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    for words in ('RAN: True', 'STATE: None', 'UNMAPPED: True', 'CORE: True'):
        assert words in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize('sep,tau', [('dot-softmax-orig', None), ('dot-sigmoid-orig', 12.5)])
def test_infer_past_the_hold_is_the_restatement_on_the_models_embedding(hp, sep, tau):
    from danet_amd import ops
    T, T0 = 40, 8
    src, mix = _signals(T, seed=1)
    model = _model(hp, INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=T0, ONLINE_MEMORY_FRAMES=tau,
                   SEPARATOR_TYPE=sep, DEBUG=True)
    lam = 1.0 if tau is None else float(np.exp(-1.0 / tau))
    assert model.online[0] == T0 and abs(model.online[1] - lam) <= 1e-15
    got = model.infer(mix)
    assert tuple(got.shape) == (2, 2, T, 33) and got.dtype == torch.complex64
    traj = model.valid_estimator.debug_fetches['attr_trajectory'].cpu().numpy()
    with torch.no_grad():
        fe = ops.frontend(mix[:, None].contiguous())
        emb = model.encoder(fe['mix_log'])
        a0, _, _ = ops.AnchorAttractorFn.apply(emb[:, :T0].contiguous(), model.vars['global/infer_estimator/anchors'], 2)
    V, W, A0 = emb.cpu().numpy(), fe['mix_pwr'].cpu().numpy(), a0.cpu().numpy()
    act = model.separator.ACT
    want_traj = OR.attractors(V, W, A0, act, lam, T0, float(hp.EPS))
    assert tuple(traj.shape) == (2, T, 2, 4) and _rel(traj, want_traj) <= OR.BAR
    assert np.array_equal(traj[:, :T0], np.broadcast_to(A0[:, None], traj[:, :T0].shape))
    want = OR.separate(V, W, want_traj, act)
    assert _rel(got.abs().cpu().numpy(), want) <= OR.BAR
    # and it is not what one attractor set gives
    anchor = _model(hp, INFER_ESTIMATOR_METHOD='anchor', SEPARATOR_TYPE=sep).infer(mix)
    assert _rel(anchor.abs().cpu().numpy(), want) > 1e-3
    check_lstm_status()


def test_valid_step_returns_its_usual_keys(hp):
    src, mix = _signals(40, seed=2)
    model = _model(hp, INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=8)
    res = model.valid_step(src)
    assert list(res) == ['loss', 'SNR'] and all(np.isfinite(float(v)) for v in res.values())
    model = _model(hp, INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=8, EVAL_SI_SDR=True)
    res2 = model.valid_step(src)
    assert list(res2) == ['loss', 'SNR', 'SI-SDR', 'SI-SDRi'] and all(np.isfinite(float(v)) for v in res2.values())
    assert float(res2['loss']) == float(res['loss']) and float(res2['SNR']) == float(res['SNR'])
    with torch.no_grad():
        out = model.forward(src, with_valid=True, with_train=False)
    assert tuple(out['valid_attrs'].shape) == (2, 40, 2, 4) and tuple(out['sep_pwr_valid'].shape) == (2, 2, 40, 33)
    # a train step of the same model still runs: the train branch never sees the estimator
    assert np.isfinite(float(model.train_step(src)['loss']))
    check_lstm_status()


def test_demo_mode_runs_end_to_end(hp, tmp_path, monkeypatch):
    import scipy.io.wavfile
    from danet_amd import _lib, cli, datasets, utils
    monkeypatch.chdir(tmp_path)
    cfg = dict(TINY, BATCH_SIZE=4, DATASET_TYPE='synth', INFER_ESTIMATOR_METHOD='online', ONLINE_INIT_FRAMES=8,
               ONLINE_MEMORY_FRAMES=50)
    (tmp_path / 'cfg.json').write_text(json.dumps(cfg))
    wave = (datasets.speech_shaped_wave(np.random.RandomState(2), 8000, 8000)).astype(np.int16)
    scipy.io.wavfile.write('mix.wav', 8000, wave)
    model = cli.main(['-n', 'tracked', '-m', 'demo', '-if', 'mix.wav', '-c', 'cfg.json'], out=io.StringIO())
    assert model.online == (8, math.exp(-1.0 / 50)) and hp.BATCH_SIZE == 1 and _lib._online is not None
    x = torch.as_tensor(utils.load_wavfile('mix.wav').astype(np.complex64)).to(model.device)[None]
    assert x.shape[1] > 8
    sep = model.infer(x)
    model.check_status()
    for i in (1, 2):
        sr, y = scipy.io.wavfile.read('mix_separated_%d.wav' % i)
        assert sr == 8000 and np.isfinite(y).all() and np.abs(y).max() > 0
        utils.save_wavfile('direct_%d.wav' % i, sep[0, i - 1].cpu().numpy())
        assert open('direct_%d.wav' % i, 'rb').read() == open('mix_separated_%d.wav' % i, 'rb').read()
    check_lstm_status()
