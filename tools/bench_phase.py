'''
What the MISI phase refinement (PHASE_REFINE_ITERS) costs, measured in ONE process on one box with INTERLEAVED blocks;
prints one JSON line and writes it to profiles/phase_bench.json.  Every row carries the per-block figures, their median
and the block-to-block spread (max - min): a difference inside the spread counts as equal.  No bar is set: the
expectation is launch-bound, a few launch floors per iteration, and the figures say whether that holds.

  (a) the three entry points and one full iteration (synth + project) through the C entry points, --reps back-to-back
      calls between two events per block, us per call, next to the launch floor of the same run (danet_phase_synth on
      the smallest shape of the envelope), at two shapes (B, C, T, N, S):
      (1, 2, 1251, 512, 128), the cfg-5 inference shape, and (32, 2, 128, 256, 64), the cfg-2 validation shape.
  (b) Model.infer at cfg 5 with PHASE_REFINE_ITERS = 5 against the key null.

    python tools/bench_phase.py [--rounds 5] [--reps 20] [--step-reps 5] [--out FILE]
'''
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SHAPES = {'cfg5_infer': (1, 2, 1251, 512, 128), 'cfg2_valid': (32, 2, 128, 256, 64)}
FLOOR_SHAPE = (1, 1, 2, 64, 8)


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


def _buffers(B, C, T, N, S, seed):
    import numpy as np
    import torch
    from danet_amd import ops
    rng = np.random.RandomState(seed)
    F = N // 2 + 1
    est0 = torch.as_tensor((rng.standard_normal((B, C, T, F)) + 1j * rng.standard_normal((B, C, T, F)))
                           .astype(np.complex64)).cuda()
    mix = est0.sum(1, keepdim=True).contiguous()
    w = torch.as_tensor(np.sqrt(np.hanning(N)).astype(np.float32)).cuda()
    ws = torch.zeros(ops.phase_workspace_bytes(B, C, T, N, S), dtype=torch.uint8, device='cuda')
    return est0, mix, w, ws, torch.empty_like(est0)


def entry_points_row(name, rounds, reps):
    import torch
    from danet_amd import _lib
    B, C, T, N, S = SHAPES[name]
    est0, mix, w, ws, x = _buffers(B, C, T, N, S, 0)
    f_est0, f_mix, f_w, f_ws, f_x = _buffers(*FLOOR_SHAPE, seed=1)
    lib, st, p = _lib.load_phase(), _lib.stream(), _lib.ptr
    r2 = torch.view_as_real

    def init():
        assert lib.danet_phase_init(st, B, C, 1, T, N, S, p(r2(est0)), p(r2(mix)), p(w), p(ws), p(r2(x))) == 0

    def synth():
        assert lib.danet_phase_synth(st, B, C, T, N, S, p(r2(x)), p(w), p(ws)) == 0

    def project():
        assert lib.danet_phase_project(st, B, C, T, N, S, p(w), p(ws), p(r2(x)), None) == 0

    def iteration():
        synth()
        project()

    def floor():
        assert lib.danet_phase_synth(st, *FLOOR_SHAPE, p(r2(f_x)), p(f_w), p(f_ws)) == 0
    assert lib.danet_phase_init(st, *FLOOR_SHAPE[:2], 1, *FLOOR_SHAPE[2:], p(r2(f_est0)), p(r2(f_mix)), p(f_w), p(f_ws),
                                p(r2(f_x))) == 0
    fns = dict(init_two_launches=init, synth=synth, project=project, iteration_two_launches=iteration,
               launch_floor=floor)
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(r2(x)).all())
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_timed_launches(fn, reps))
    F, Ls = N // 2 + 1, (T - 1) * S
    r = dict(shape=dict(B=B, C=C, T=T, N=N, S=S), unit='us per call, back to back, C entry point',
             # what one project launch must move at the least: the C + 1 waveforms, A, the old and the new x
             project_min_bytes=B * (C + 1) * Ls * 4 + B * C * T * F * (4 + 8 + 8))
    r.update({k: _summary(v) for k, v in t.items()})
    r['iteration_in_launch_floors'] = round(r['iteration_two_launches']['median'] / r['launch_floor']['median'], 2)
    r['project_gbytes_per_s'] = round(r['project_min_bytes'] / r['project']['median'] / 1e3, 1)
    print('%s: init %.1f, synth %.1f, project %.1f, iteration %.1f us; launch floor %.1f us (%.1f floors per iteration)'
          % ((name,) + tuple(r[k]['median'] for k in fns) + (r['iteration_in_launch_floors'],)), file=sys.stderr)
    return r


def infer_row(rounds, reps, K=5):
    import numpy as np
    import torch
    import bench
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    cfg = bench.CONFIGS['cfg5']
    base = dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam')
    rng = np.random.RandomState(2)
    F = cfg['hp']['FFT_SIZE'] // 2 + 1
    mix = torch.as_tensor((rng.standard_normal((cfg['batch'], cfg['frames'], F))
                           + 1j * rng.standard_normal((cfg['batch'], cfg['frames'], F))).astype(np.complex64)).cuda()
    models = {}
    for tag, key in (('key_null', None), ('key_%d' % K, K)):
        hparams.reset()
        hparams.load(dict(base, PHASE_REFINE_ITERS=key))
        hparams.digest()
        models[tag] = Model('bench_phase', device='cuda:0', seed=7).build()
    last = {}

    def step(tag):
        def fn():
            last[tag] = models[tag].infer(mix)
        return fn
    for _ in range(3):
        for tag in models:
            step(tag)()
    torch.cuda.synchronize()
    a, b = (last[tag].abs() for tag in models)
    assert float((a - b).abs().max()) <= 1e-6 * float(a.max())       # the same magnitudes, another phase
    t = {tag: [] for tag in models}
    for _ in range(rounds):
        for tag in models:
            t[tag].append(_timed_launches(step(tag), reps))
    for m in models.values():
        m.check_status()
    r = dict(config='cfg5', iterations=K, unit='us per Model.infer, back to back')
    r.update({tag: _summary(v) for tag, v in t.items()})
    r['added_us_per_infer'] = round(r['key_%d' % K]['median'] - r['key_null']['median'], 2)
    r['added_us_per_iteration'] = round(r['added_us_per_infer'] / K, 2)
    print('infer cfg5: key null %.1f us (spread %.1f), K = %d %.1f us (spread %.1f): +%.1f us'
          % (r['key_null']['median'], r['key_null']['spread'], K, r['key_%d' % K]['median'], r['key_%d' % K]['spread'],
             r['added_us_per_infer']), file=sys.stderr)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--step-reps', type=int, default=5)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    assert torch.cuda.is_available(), 'bench_phase.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='MISI phase refinement: init, synth, project and one iteration at two shapes, Model.infer at '
                        'cfg 5 with and without the key; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, step_reps=args.step_reps, device=torch.cuda.get_device_name(0))
    for name in SHAPES:
        res['a_' + name] = entry_points_row(name, args.rounds, args.reps)
    res['b_infer_cfg5'] = infer_row(args.rounds, args.step_reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'phase_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
