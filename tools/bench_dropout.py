'''
What DROPOUT_KEEP_PROB < 1 costs, measured in ONE process on one box; prints one JSON line and writes
it to profiles/dropout_bench.json:

  * the cfg-2 train step (bench.py's configuration, batches and model seed, through bench.py's own
    setup_hparams / make_batches / make_barrier) with keep 1.0 and keep 0.8, INTERLEAVED: after
    bench.py's initialisation and settle steps, --rounds rounds of [--steps steps at 1.0, --steps
    steps at 0.8], every block closed by one device synchronise, as bench.py closes its timed
    region.  Reported: the per-block ms/step of both settings, their medians and the ratio;
  * danet_dropout_apply alone at [4096][600] and [4096][1200] (dense, out of place and in place):
    --reps back-to-back launches between two events -> us per launch and TB/s of the 8 bytes per
    element it moves.

    python tools/bench_dropout.py [--rounds 6] [--steps 50] [--reps 200]
'''
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(reps):
    import torch
    from danet_amd import ops
    out = []
    spec = ops.DropoutSpec(0.8, 1337, 0, 0)
    for rows, cols in ((4096, 600), (4096, 1200)):
        x = torch.randn(rows, cols, device='cuda')
        y = torch.empty_like(x)
        for name, dst in (('out_of_place', y), ('in_place', x)):
            fn = lambda: ops.dropout_apply(x, dst, rows, cols, cols, cols, spec, 0)
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / reps
            out.append(dict(rows=rows, cols=cols, mode=name, us=round(us, 2),
                            tb_per_s=round(8.0 * rows * cols / us / 1e6, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--reps', type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.load_package()
    import bench
    from danet_amd import ops
    from danet_amd.model import Model
    torch.cuda.set_device(0)
    device = torch.device('cuda:0')
    cfg = bench.CONFIGS['cfg2']
    bargs = types.SimpleNamespace(batch=cfg['batch'], layers=cfg['layers'], hdim=cfg['hdim'], frames=cfg['frames'])
    hp = bench.setup_hparams(bargs, cfg)
    batches = bench.make_batches(hp, 0, 4, device)
    model = Model('bench', device=device, seed=1337).build()
    barrier = bench.make_barrier(False)

    def block(keep, n):
        hp.DROPOUT_KEEP_PROB = keep
        barrier()
        t0 = time.perf_counter()
        for i in range(n):
            model.train_step(batches[i % len(batches)])
        barrier()
        return (time.perf_counter() - t0) * 1e3 / n

    for keep in (1.0, 0.8):            # initialisation + settle, both paths (bench.py: 1 + 8 steps)
        block(keep, 9)
    ms = {1.0: [], 0.8: []}
    for _ in range(args.rounds):
        for keep in (1.0, 0.8):
            ms[keep].append(block(keep, args.steps))
    assert ops.lstm_status_ok()
    off, on = float(np.median(ms[1.0])), float(np.median(ms[0.8]))
    res = dict(workload='cfg2 train step, DROPOUT_KEEP_PROB 1.0 vs 0.8, interleaved blocks in one process',
               rounds=args.rounds, steps_per_block=args.steps,
               keep_1_0_ms_per_step=[round(v, 4) for v in ms[1.0]],
               keep_0_8_ms_per_step=[round(v, 4) for v in ms[0.8]],
               keep_1_0_median_ms=round(off, 4), keep_0_8_median_ms=round(on, 4),
               on_cost_percent=round(100.0 * (on / off - 1.0), 2),
               dropout_launches_per_step=2 * cfg['layers'],
               apply_kernel=kernel_times(args.reps))
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'dropout_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
