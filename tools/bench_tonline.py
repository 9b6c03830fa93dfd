'''
What training for streaming (TRAIN_ESTIMATOR_METHOD = "truth-online") costs, measured in ONE process on one box with
INTERLEAVED blocks; prints one JSON line and writes it to profiles/tonline_bench.json.  Every row carries the per-block
figures, their median and the block-to-block spread (max - min).

  (a) each of the five entry points of libdanet_tonline_hip.so through the C ABI at the cfg-2 head shapes (B = 32,
      C = 2, T = 128, F = 129, E = 20), --reps launches back to back between two events per block, us per launch;
      beside them danet_online_separate (the forward of the separator) and, as the launch floor of the same run,
      danet_tonline_scan on one utterance of one frame;
  (b) Model.train_step at cfg 2 with ENCODER_TYPE = "lstm-orig": "truth-online" / "online" against "truth-weighted" /
      "anchor", two models built in this process from the same seed, --steps steps per block, ms per step.

No bar is set on either: the figures are what they are, and the README says where the difference goes.

    python tools/bench_tonline.py [--rounds 5] [--reps 50] [--steps 20] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(B=32, C=2, T=128, F=129, E=20)
LAMBDA, T0, EPS = 0.99, 32, 1e-7
CFG2 = dict(BATCH_SIZE=32, NUM_LSTM_LAYERS=3, LSTM_HDIM=300, MAX_TRAIN_LEN=128, ENCODER_TYPE='lstm-orig',
            OPTIMIZER_TYPE='adam', MAX_N_SIGNAL=2, FFT_SIZE=256, FFT_STRIDE=64, SMPRATE=8000, EMBED_SIZE=20,
            NUM_ANCHOR=6, SEPARATOR_TYPE='dot-softmax-orig')
PAIRS = {'truth_online__online': dict(TRAIN_ESTIMATOR_METHOD='truth-online', INFER_ESTIMATOR_METHOD='online'),
         'truth_weighted__anchor': dict(TRAIN_ESTIMATOR_METHOD='truth-weighted', INFER_ESTIMATOR_METHOD='anchor')}


def _summary(blocks):
    import numpy as np
    return dict(blocks=[round(float(v), 4) for v in blocks], median=round(float(np.median(blocks)), 4),
                spread=round(float(max(blocks) - min(blocks)), 4))


def _timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps                 # ms per call


def entry_point_rows(rounds, reps):
    import torch
    from danet_amd import _lib
    B, C, T, F, E = (SHAPE[k] for k in 'BCTFE')
    lib, on, st = _lib.load_tonline(), _lib.load_online(), _lib.stream()
    f32 = lambda *s: torch.randn(*s, device='cuda')
    embed, w, src_pwr = f32(B, T, F, E), f32(B, T, F).abs(), f32(B, C, T, F).abs()
    dout, dattr = f32(B, C, T, F), f32(B, T, C, E)
    s, q, attr, r, da = f32(B, T, C, E), f32(B, T, C), f32(B, T, C, E), f32(B, T, C, E), f32(B, T, C, E)
    den = torch.empty(B, T, C, dtype=torch.float64, device='cuda')
    dv, out = f32(B, T, F, E), f32(B, C, T, F)
    p = lambda t: t.data_ptr()
    calls = {
        'frame_sums': lambda: lib.danet_tonline_frame_sums(st, B, C, T, F, E, p(embed), p(src_pwr), p(w), p(s), p(q)),
        'scan': lambda: lib.danet_tonline_scan(st, B, C, T, E, LAMBDA, T0, EPS, p(s), p(q), p(attr), p(den)),
        'scan_bwd': lambda: lib.danet_tonline_scan_bwd(st, B, C, T, E, LAMBDA, T0, p(dattr), p(den), p(r)),
        'sums_bwd': lambda: lib.danet_tonline_sums_bwd(st, B, C, T, F, E, p(src_pwr), p(w), p(r), p(dv)),
        'separate_bwd': lambda: lib.danet_tonline_separate_bwd(st, 0, B, C, T, F, E, p(w), p(attr), p(embed), p(dout),
                                                               p(dv), p(da)),
        'online_separate': lambda: on.danet_online_separate(st, 0, B, C, T, F, E, p(w), p(attr), p(embed), p(out)),
        'launch_floor': lambda: lib.danet_tonline_scan(st, 1, 1, 1, 1, LAMBDA, T0, EPS, p(s), p(q), p(attr), p(den)),
    }
    for fn in calls.values():                        # in dependency order: den exists before scan_bwd reads it
        assert fn() == 0
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(1e3 * _timed(fn, reps))
    rows = dict(shape=SHAPE, unit='us per launch, %d launches back to back between two events' % reps,
                embed_bytes=4 * B * T * F * E)
    rows.update({k: _summary(v) for k, v in t.items()})
    print('us per launch: %s' % ', '.join('%s %.1f' % (k, rows[k]['median']) for k in calls), file=sys.stderr)
    return rows


def train_step_rows(rounds, steps):
    import torch
    import bench
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    models = {}
    for name, pair in PAIRS.items():
        hparams.reset()
        hparams.load(dict(CFG2, **pair))
        hparams.digest()
        models[name] = Model(name, device='cuda:0', seed=1).build()
    batches = bench.make_batches(hparams, 0, 2, torch.device('cuda:0'))
    state = {'i': 0}

    def step_of(model):
        def step():
            model.train_step(batches[state['i'] % len(batches)], sync_metrics=False)
            state['i'] += 1
        return step
    steppers = {name: step_of(m) for name, m in models.items()}
    for fn in steppers.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in steppers}
    for _ in range(rounds):
        for k, fn in steppers.items():
            t[k].append(_timed(fn, steps))
    rows = dict(config=dict(CFG2), unit='ms per train step, %d steps between two events' % steps)
    rows.update({k: _summary(v) for k, v in t.items()})
    rows['difference_ms'] = round(rows['truth_online__online']['median'] - rows['truth_weighted__anchor']['median'], 4)
    print('ms per step: %s' % ', '.join('%s %.3f' % (k, rows[k]['median']) for k in steppers), file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_tonline.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='truth-online: the five entry points at the cfg-2 head shapes beside the launch floor, and the '
                        'cfg-2 lstm-orig train step against truth-weighted / anchor; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, steps=args.steps, device=torch.cuda.get_device_name(0))
    res['entry_points'] = entry_point_rows(args.rounds, args.reps)
    res['train_step'] = train_step_rows(args.rounds, args.steps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'tonline_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
