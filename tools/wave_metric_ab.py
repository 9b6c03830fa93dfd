'''
A/B of the three libraries that share csrc/wave_metric.h (metric, neval, wavloss): run ONE process per directory of
builds and compare what the processes print.

    python tools/wave_metric_ab.py DIR            # sha256 of every output on seeded inputs, one line each
    python tools/wave_metric_ab.py DIR --time     # us per launch of the eight labels, one JSON line

DIR holds libdanet_metric_hip.so, libdanet_neval_hip.so and libdanet_wavloss_hip.so (danet-tensorflow_amd/csrc for
the tree's own); the three paths of _lib are assigned before anything maps a library.

Digests.  Inputs from numpy.random.default_rng(seed).  Synthesis shapes (N, S) where the tiling can go wrong --
(64, 8): q = 4, r = 0; (64, 24): r != 0; (256, 96): r != 0, q = 1; (1024, 512): fewest frames per tile -- each at
T = 2, T = 3 and the T of exactly two tiles with a one-hop last one, B = 2, C in (1, 4); neval with gains and with
gain None; wavloss_bwd in both output forms with one pair entry of -1.  Two builds compute the same thing when
their listings are equal.

Times.  The evaluation shape of the default hparams (B 32, C 2, T 128, N 256, S 64): --blocks blocks of --reps
chains of the eight launches under _lib.profile_start(only=labels); per label the blocks' us per launch, their
median and spread.  Alternate the directories between processes and read a difference against the spread of two
runs of the same directory.
'''
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 8), (64, 24), (256, 96), (1024, 512))
LABELS = ('metric_synth', 'metric_gram', 'metric_si_sdr', 'neval_synth', 'neval_gram', 'neval_si_sdr', 'wavloss_fwd',
          'wavloss_bwd')


def max_hops(N, S):
    '''tiling_of (csrc/wave_metric.h): the hops of a full tile'''
    max_frames = min(32, 16384 // N - 1)
    q, r = (N // 2) // S, (N // 2) % S
    return max_frames - (2 * q - 1 if r == 0 else 2 * q + 1)


def _spectra(rng, *shape):
    import numpy as np
    import torch
    return torch.from_numpy((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)).cuda()


def _inputs(rng, B, C, T, N):
    import numpy as np
    import torch
    F = N // 2 + 1
    src = _spectra(rng, B, C, T, F)
    est = _spectra(rng, B, C, T, F) * 0.3 + src.flip(1)
    noise = _spectra(rng, B, T, F)
    gain = torch.from_numpy(rng.uniform(0.05, 3.0, B).astype(np.float32)).cuda()
    window = torch.from_numpy(np.sqrt(np.hanning(N + 1)[:N]).astype(np.float32)).cuda()
    ang = rng.uniform(-np.pi, np.pi, (B, T, F))
    phasor = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)).cuda()
    dloss = torch.from_numpy(rng.uniform(0.5, 2.0, 1).astype(np.float32)).cuda()
    return src, est, noise, gain, window, phasor, dloss


def digests(seed):
    import numpy as np
    import torch
    from danet_amd import ops
    rng = np.random.default_rng(seed)

    def show(label, *tensors):
        h = hashlib.sha256()
        for t in tensors:
            t = torch.view_as_real(t) if t.is_complex() else t
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        print('%-44s %s' % (label, h.hexdigest()))

    B = 2
    for N, S in SHAPES:
        for T in (2, 3, max_hops(N, S) + 2):
            for C in (1, 4):
                src, est, noise, gain, window, phasor, dloss = _inputs(rng, B, C, T, N)
                at = 'N%d S%d T%d C%d ' % (N, S, T, C)
                wav = ops.metric_synth(src, est, S, window=window)
                G = ops.metric_gram(wav)
                show(at + 'metric_synth', wav)
                show(at + 'metric_gram', G)
                show(at + 'metric_finalize', *ops.metric_finalize(G))
                for name, g in (('gain', gain), ('nogain', None)):
                    nwav = ops.neval_synth(src, est, noise, g, S, window=window)
                    nG = ops.neval_gram(nwav)
                    show(at + 'neval_synth ' + name, nwav)
                    show(at + 'neval_gram ' + name, nG)
                    show(at + 'neval_finalize ' + name, *ops.neval_finalize(nG))
                fwd = ops.wavloss_fwd(G)
                show(at + 'wavloss_fwd', *fwd)
                pair, coef = fwd[4].clone(), fwd[5]
                pair[B - 1, C - 1] = -1
                show(at + 'wavloss_bwd complex', ops.wavloss_bwd(wav, pair, coef, N, S, window=window, dloss=dloss))
                show(at + 'wavloss_bwd real', ops.wavloss_bwd(wav, pair, coef, N, S, window=window, phasor=phasor))
    torch.cuda.synchronize()


def times(seed, blocks, reps, B=32, C=2, T=128, N=256, S=64):
    import numpy as np
    import torch
    from danet_amd import _lib, ops
    rng = np.random.default_rng(seed)
    src, est, noise, gain, window, phasor, _ = _inputs(rng, B, C, T, N)
    Ls = (T - 1) * S
    wav = torch.empty(B, 2 * C, Ls, dtype=torch.float32, device='cuda')
    nwav = torch.empty(B, 2 * C + 1, Ls, dtype=torch.float32, device='cuda')
    G, nG = ops.metric_gram(ops.metric_synth(src, est, S, window=window)), None
    out2, out3, outf = ops.metric_finalize(G), None, ops.wavloss_fwd(G)
    dsep = torch.empty(B, C, T, N // 2 + 1, dtype=torch.float32, device='cuda')

    def chain():
        nonlocal nG, out3
        ops.metric_synth(src, est, S, window=window, out=wav)
        ops.metric_gram(wav, out=G)
        ops.metric_finalize(G, out=(out2[1], out2[2], out2[0]))
        ops.neval_synth(src, est, noise, gain, S, window=window, out=nwav)
        nG = ops.neval_gram(nwav, out=nG)
        out3 = ops.neval_finalize(nG, out=None if out3 is None else (out3[1], out3[2], out3[0]))
        ops.wavloss_fwd(G, out=outf)
        ops.wavloss_bwd(wav, outf[4], outf[5], N, S, window=window, phasor=phasor, out=dsep)

    for _ in range(50):
        chain()
    torch.cuda.synchronize()
    per = {k: [] for k in LABELS}
    for _ in range(blocks):
        _lib.profile_start(only=LABELS)
        for _ in range(reps):
            chain()
        for k, (n, ms) in _lib.profile_stop().items():
            assert n == reps, (k, n)
            per[k].append(ms * 1e3 / n)
    res = dict(shape=dict(B=B, C=C, T=T, N=N, S=S), unit='us per launch, event pair around the call', blocks=blocks,
               reps=reps)
    for k in LABELS:
        res[k] = dict(blocks=[round(v, 3) for v in per[k]], median=round(float(np.median(per[k])), 3),
                      spread=round(max(per[k]) - min(per[k]), 3))
    print(json.dumps(res))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('dir', help='directory of libdanet_{metric,neval,wavloss}_hip.so')
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--seed', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    from danet_amd import _lib
    for name in ('metric', 'neval', 'wavloss'):
        path = os.path.join(os.path.abspath(args.dir), 'libdanet_%s_hip.so' % name)
        assert os.path.isfile(path), path
        setattr(_lib, name.upper() + '_LIB_PATH', path)
    assert torch.cuda.is_available(), 'wave_metric_ab.py runs on the GPU'
    torch.cuda.set_device(0)
    print('# %s' % ('times' if args.time else 'digests'), file=sys.stderr)
    if args.time:
        times(args.seed, args.blocks, args.reps)
    else:
        digests(args.seed)
