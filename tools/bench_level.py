'''
What the active-speech-level measurement of the wavdir dataset (MIX_LEVEL_MEASURE = "active") costs, measured in
ONE process on one box with INTERLEAVED blocks; prints one JSON line and writes it to profiles/level_bench.json.
Every row carries the per-block figures, their median and the block-to-block spread (max - min).

  (a) danet_level_activity over the synthetic pool of tools/bench_mix.py (--rows utterances of 1 .. 10 s at 8 kHz
      plus two of 5e6 samples, laid back to back, gated to 50 % activity), in the launches the dataset makes
      (WavDirData.level_chunks, 64 MiB of workspace): --reps passes over the WHOLE pool through the C entry point
      between two events per block, ms per pass and samples per second; next to it, as the yardstick of the same
      run, danet_mix_power over the same bytes;
  (b) the scipy `lfilter` restatement of the envelope plus the 16 vectorised counts (tests/level_ref.py) on a 10 s
      slice of the pool on ONE host core, scaled to the pool's length: what the host would cost.

No bar is set: the kernel runs once per pool.  The counts of three rows are checked against the restatement, so
that the timed thing is known to be the right thing.

    python tools/bench_level.py [--rounds 5] [--reps 3] [--rows 2000] [--out FILE]
'''
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


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
    return a.elapsed_time(b) / reps                 # ms per pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=2000)
    ap.add_argument('--out', help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.load_package()
    import level_ref as LR
    from danet_amd import _lib, ops
    from danet_amd.datasets import WavDirData
    assert torch.cuda.is_available(), 'bench_level.py measures on the GPU'
    torch.cuda.set_device(0)
    fs = 8000
    rng = np.random.RandomState(0)
    lens = np.concatenate([rng.randint(8000, 80001, size=args.rows), [5 * 10 ** 6, 5 * 10 ** 6]]).astype(np.int64)
    rng.shuffle(lens)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    total = int(lens.sum())
    pool = torch.empty(total, dtype=torch.float32, device='cuda')
    for lo in range(0, total, 1 << 24):             # noise gated in 0.5 s steps to about half activity, -50 dB floor
        n = min(1 << 24, total - lo)
        gate = (torch.rand((n + 3999) // 4000, device='cuda') < 0.5).float().repeat_interleave(4000)[:n]
        pool[lo:lo + n] = torch.randn(n, device='cuda') * 1000.0 * torch.clamp(gate, min=10.0 ** -2.5)
    gg, hang = WavDirData.level_params(fs)
    sums = ops.mix_power(pool, offs, lens).cpu().numpy()
    thr = WavDirData.level_thresholds(sums / lens)
    chunks = list(WavDirData.level_chunks(lens, WavDirData.LEVEL_WS_BYTES))
    counts = np.zeros((len(lens), 16), np.int64)
    for rows in chunks:
        counts[rows] = ops.level_activity(pool, offs[rows], lens[rows], thr[rows], gg, hang).cpu().numpy()
    active = WavDirData.active_power(sums, lens, counts, thr)
    checked = []
    for u in (0, 1, int(np.argmin(lens))):
        x = pool[int(offs[u]):int(offs[u] + lens[u])].cpu().numpy()
        want = LR.counts(LR.envelope(x, gg), thr[u], hang)
        checked.append(bool(np.array_equal(want, counts[u])))
    assert all(checked), checked

    lib, mix, st = _lib.load_level(), _lib.load_mix(), _lib.stream()
    o, l, t = torch.from_numpy(offs).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(thr).cuda()
    plans, ws_max = [], 16
    for rows in chunks:
        idx = torch.from_numpy(rows).cuda()
        max_len = int(lens[rows].max())
        nbytes = lib.danet_level_workspace_bytes(len(rows), max_len)
        ws_max = max(ws_max, nbytes)
        plans.append((len(rows), o[idx].contiguous(), l[idx].contiguous(), max_len, t[idx].contiguous(),
                      torch.empty(len(rows), 16, dtype=torch.int64, device='cuda'), nbytes))
    ws = torch.empty(ws_max, dtype=torch.uint8, device='cuda')
    max_all = int(lens.max())
    mbytes = mix.danet_mix_workspace_bytes(len(lens), max_all)
    mws = torch.zeros(max(mbytes, 8), dtype=torch.uint8, device='cuda')
    mout = torch.empty(len(lens), dtype=torch.float64, device='cuda')

    def level():
        for n, oo, ll, max_len, tt, out, nbytes in plans:
            assert lib.danet_level_activity(st, n, pool.data_ptr(), total, oo.data_ptr(), ll.data_ptr(), max_len, gg,
                                            hang, tt.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes) == 0

    def power():
        assert mix.danet_mix_power(st, len(lens), pool.data_ptr(), total, o.data_ptr(), l.data_ptr(), max_all,
                                   mout.data_ptr(), mws.data_ptr(), mbytes) == 0
    for _ in range(2):
        level()
        power()
    torch.cuda.synchronize()
    for rows, plan in zip(chunks, plans):
        assert np.array_equal(plan[5].cpu().numpy(), counts[rows])      # two routes, the same counts
    t_level, t_power = [], []
    for _ in range(args.rounds):
        t_level.append(_timed(level, args.reps))
        t_power.append(_timed(power, args.reps * 10))

    # (b) the host: one 10 s slice, envelope + 16 counts, scaled to the pool
    x = pool[:10 * fs].cpu().numpy()
    th = LR.thresholds(LR.sum_squares(x) / len(x))
    t_host = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        LR.counts(LR.envelope(x, gg), th, hang)
        t_host.append((time.perf_counter() - t0) * 1e3)
    res = dict(workload='wavdir active speech level: P.56 activity counts of a pool; interleaved blocks in one process',
               rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0), smprate=fs,
               rows=len(lens), samples=total, pool_bytes=4 * total, longest_row=max_all, shortest_row=int(lens.min()),
               launches_of_rows=len(chunks), kernel_launches_per_pass=4 * len(chunks), workspace_bytes=int(ws_max),
               counts_checked_against_restatement_on_3_rows=checked,
               median_active_over_mean_dB=round(float(np.median(10 * np.log10(active / (sums / lens)))), 3),
               unit='ms per pass over the whole pool, C entry point',
               level_activity=_summary(t_level), mix_power=_summary(t_power),
               host_lfilter_10s_slice_ms=_summary(t_host))
    res['level_activity_Msamples_per_s'] = round(total / (res['level_activity']['median'] * 1e-3) / 1e6, 1)
    res['mix_power_GBps'] = round(4 * total / (res['mix_power']['median'] * 1e-3) / 1e9, 1)
    res['host_scaled_to_pool_s'] = round(res['host_lfilter_10s_slice_ms']['median'] * 1e-3 * total / len(x), 2)
    print('level: %d rows, %.1f M samples: %.2f ms per pass (spread %.2f) = %.0f Msamples/s; mix_power %.3f ms; host '
          'restatement scaled: %.1f s' % (len(lens), 1e-6 * total, res['level_activity']['median'],
                                         res['level_activity']['spread'], res['level_activity_Msamples_per_s'],
                                         res['mix_power']['median'], res['host_scaled_to_pool_s']), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'level_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
