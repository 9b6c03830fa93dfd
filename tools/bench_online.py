'''
What the online attractor estimator (INFER_ESTIMATOR_METHOD = "online") costs, measured in ONE process on one box with
INTERLEAVED blocks; prints one JSON line and writes it to profiles/online_bench.json.  Every row carries the per-block
figures, their median and the block-to-block spread (max - min): a difference inside the spread counts as equal.  No
bar is set: the scan is new and latency-bound (one workgroup per utterance walks the frames), and the figures say what
a frame costs.

  The scan (danet_online_scan, from a fresh state), danet_online_separate and danet_online_init through the C entry
  points, --reps back-to-back calls between two events per block, us per call and, for the scan, us per frame; next
  to them, as the yardstick of the same run on the same tensors, danet_attractor_anchor_fwd + danet_separate_fwd (ONE
  attractor set per recording).  Two shapes (B, T, F, E, C): (1, 1251, 257, 20, 2), the cfg-5 inference shape, and
  (32, 128, 129, 20, 2), the cfg-2 validation shape.

  The scan alone, us per frame, at B = 1 and T = 400 over a set of (F, E, C) that separates what a frame costs: the
  fixed part (F = 1), the part that grows with the bins (F = 64 .. 513, with 256 and 257 either side of a second bin
  per thread), and with the row (E = 4, 19, 20, 64) and the sources (C = 4).

    python tools/bench_online.py [--rounds 5] [--reps 20] [--out FILE]
'''
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {'cfg5_infer': (1, 1251, 257, 20, 2), 'cfg2_valid': (32, 128, 129, 20, 2)}
NUM_ANCHOR, T0, TAU, EPS = 6, 32, 100.0, 1e-7
PROBE_T = 400
PROBE_SHAPES = [(1, 20, 2), (64, 20, 2), (129, 20, 2), (256, 20, 2), (257, 20, 2), (513, 20, 2), (257, 4, 2),
                (257, 19, 2), (257, 64, 2), (257, 20, 4)]              # (F, E, C)


def clustered_inputs(B, T, F, E, C, seed):
    '''(V [B, T, F, E], W [B, T, F], A0 [B, C, E]) float32 on the device: C centres of unit-normal entries per
    utterance, every bin a centre plus 0.5 x noise, A0 = the centres plus 0.3 x noise, W = 10 |N(0, 1)| -- embeddings
    on which the update contracts, so that a long run stays finite'''
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((B, C, E))
    which = rng.randint(C, size=(B, T, F))
    V = centres[np.arange(B)[:, None, None], which] + 0.5 * rng.standard_normal((B, T, F, E))
    A0 = centres + 0.3 * rng.standard_normal((B, C, E))
    W = 10 * np.abs(rng.standard_normal((B, T, F)))
    return tuple(torch.as_tensor(x.astype(np.float32)).cuda() for x in (V, W, A0))


def _summary(blocks):
    import numpy as np
    return dict(blocks=[round(float(v), 3) for v in blocks], median=round(float(np.median(blocks)), 3),
                spread=round(float(max(blocks) - min(blocks)), 3))


def _timed_launches(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def shape_row(name, rounds, reps, act=1):
    import numpy as np
    import torch
    from danet_amd import _lib, ops
    B, T, F, E, C = SHAPES[name]
    V, W, A0 = clustered_inputs(B, T, F, E, C, seed=7)
    anchors = torch.as_tensor(np.random.RandomState(1).standard_normal((NUM_ANCHOR, E)).astype(np.float32)).cuda()
    lam, N, P = math.exp(-1.0 / TAU), T * F, math.comb(NUM_ANCHOR, C)
    state = torch.empty(B, ops.online_state_bytes(C, E) // 8, dtype=torch.float64, device='cuda')
    traj = torch.empty(B, T, C, E, device='cuda')
    out = torch.empty(B, C, T, F, device='cuda')
    attr, asets = torch.empty(B, C, E, device='cuda'), torch.empty(B, P, C, E, device='cuda')
    asum, choice = torch.empty(B, P, C, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')
    ws = torch.zeros(_lib.ws_bytes(_lib.WS_ATTRACTOR_ANCHOR, B, C, N, E, NUM_ANCHOR), dtype=torch.uint8, device='cuda')
    on, core, st, p = _lib.load_online(), _lib.load(), _lib.stream(), _lib.ptr

    def init():
        assert on.danet_online_init(st, B, C, E, p(A0), p(state)) == 0

    def scan():                                    # the state keeps running: every call is T more frames of the track
        assert on.danet_online_scan(st, B, C, T, F, E, act, lam, T0, 0, EPS, p(V), p(W), p(state), p(traj)) == 0

    def separate():
        assert on.danet_online_separate(st, act, B, C, T, F, E, p(W), p(traj), p(V), p(out)) == 0

    def online():
        init()
        scan()
        separate()

    def anchor_fwd():
        assert core.danet_attractor_anchor_fwd(st, B, C, N, E, NUM_ANCHOR, p(V), p(anchors), p(attr), p(asets), p(asum),
                                               p(choice), p(ws), ws.numel()) == 0

    def separate_fwd():
        assert core.danet_separate_fwd(st, act, B, C, N, E, p(W), p(attr), p(V), p(out), None) == 0

    def yardstick():
        anchor_fwd()
        separate_fwd()

    fns = dict(init=init, scan=scan, separate=separate, online_three_launches=online, anchor_fwd=anchor_fwd,
               separate_fwd=separate_fwd, yardstick_anchor_plus_separate=yardstick)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(traj).all()) and bool(torch.isfinite(out).all())
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    r = dict(shape=dict(B=B, T=T, F=F, E=E, C=C), act=act, T0=T0, memory_frames=TAU,
             unit='us per call, back to back, C entry point', embedding_bytes=B * T * F * E * 4)
    r.update({k: _summary(v) for k, v in t.items()})
    r['scan_us_per_frame'] = round(r['scan']['median'] / T, 3)
    r['separate_gbytes_per_s'] = round((B * T * F * (E + 1 + C) * 4) / r['separate']['median'] / 1e3, 1)
    r['online_over_yardstick'] = round(r['online_three_launches']['median']
                                       / r['yardstick_anchor_plus_separate']['median'], 2)
    print('%s: init %.1f, scan %.1f (%.3f us per frame), separate %.1f, all three %.1f us; anchor_fwd %.1f + '
          'separate_fwd %.1f = %.1f us' % (name, r['init']['median'], r['scan']['median'], r['scan_us_per_frame'],
                                          r['separate']['median'], r['online_three_launches']['median'],
                                          r['anchor_fwd']['median'], r['separate_fwd']['median'],
                                          r['yardstick_anchor_plus_separate']['median']), file=sys.stderr)
    return r


def probe_rows(rounds, reps, act=1):
    '''the scan alone at B = 1, T = PROBE_T over PROBE_SHAPES -> {'F..E..C..': summary in us per frame}'''
    import torch
    from danet_amd import _lib, ops
    on, st, p = _lib.load_online(), _lib.stream(), _lib.ptr
    lam, cases = math.exp(-1.0 / TAU), {}
    for F, E, C in PROBE_SHAPES:
        V, W, A0 = clustered_inputs(1, PROBE_T, F, E, C, seed=F + E + C)
        state, traj = ops.online_init(A0), torch.empty(1, PROBE_T, C, E, device='cuda')

        def scan(V=V, W=W, state=state, traj=traj, F=F, E=E, C=C):
            assert on.danet_online_scan(st, 1, C, PROBE_T, F, E, act, lam, T0, 0, EPS, p(V), p(W), p(state), p(traj)) == 0
        cases['F%d_E%d_C%d' % (F, E, C)] = scan
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(_timed_launches(fn, reps) / PROBE_T)
    r = dict(B=1, T=PROBE_T, act=act, unit='us per frame of danet_online_scan, back to back')
    r.update({k: _summary(v) for k, v in t.items()})
    print('scan us per frame at B = 1, T = %d: %s' % (PROBE_T, ', '.join('%s %.2f' % (k, r[k]['median']) for k in cases)),
          file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_online.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='online attractor estimator: init, scan and separate at two shapes next to anchor_fwd + '
                        'separate_fwd on the same tensors, and the scan alone per frame over a set of shapes; '
                        'interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    for name in SHAPES:
        res[name] = shape_row(name, args.rounds, args.reps)
    res['scan_per_frame'] = probe_rows(args.rounds, max(1, args.reps // 4))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'online_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
