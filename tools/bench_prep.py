'''
What the wavdir dataset's front-end costs, measured in ONE process on one box with INTERLEAVED blocks;
prints one JSON line and writes it to profiles/prep_bench.json.  Every row carries the per-block
figures, their median and the block-to-block spread (max - min): a difference inside the spread
counts as equal.

  (a) the ragged-batch kernel (ops.stft_batch) on 64 equal-length utterances of 8128 samples at
      N = 256 / S = 64, next to danet_stft on the same samples: --reps back-to-back launches between two
      events per block, both through their C entry points with prepared arguments (the Python wrappers
      would add more host time per call than either kernel runs);
  (b) the same for one 160000-sample utterance at N = 512 / S = 128;
  (c) a 64-utterance variable-length batch through WavDirData.epoch_device (crop to 128 frames), next
      to the route such data took before (per utterance utils.stft + .cpu(), utils.random_zeropad,
      np.stack, feed.BatchFeed -- what the synth-varlen dataset does): host clock around a whole epoch
      that ends in a device synchronise, ms per batch;
  (d) cli.train_epoch over wavdir next to cli.train_epoch over synth at the cfg-2 shapes, ms per step.

(a) and (b) are the bar: the new kernel must not be slower than danet_stft in the same run.
(c) and (d) are reported.  The WAV tree of (c) and (d) is generated into a temporary folder.

    python tools/bench_prep.py [--rounds 7] [--reps 200] [--epochs 3] [--files 512] [--out FILE]
'''
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(blocks):
    import numpy as np
    return dict(blocks=[round(float(v), 4) for v in blocks], median=round(float(np.median(blocks)), 4),
                spread=round(float(max(blocks) - min(blocks)), 4))


def _timed_launches(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per launch


def kernel_row(n_utt, Ls, N, S, rounds, reps):
    import numpy as np
    import torch
    from danet_amd import ops
    from danet_amd.hparams import hparams
    hparams.reset()
    hparams.load(dict(FFT_SIZE=N, FFT_STRIDE=S))
    hparams.digest()
    window = torch.as_tensor(np.asarray(hparams.FFT_WND, dtype=np.float32)).cuda()
    x = (torch.randn(n_utt, Ls, device='cuda') * 1000).contiguous()
    T = ops.prep_num_frames(Ls, N, S)
    desc = ops.prep_desc([u * Ls for u in range(n_utt)], [Ls] * n_utt, [0] * n_utt, T, n_utt * Ls, N, S)
    desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    out = torch.empty(n_utt, T, N // 2 + 1, dtype=torch.complex64, device='cuda')
    pool = x.view(-1)
    ref = ops.stft(x, window, N, S)
    got = ops.stft_batch(pool, desc, T, window, N, S, out=out)       # (also builds and caches the plan)
    # The timed calls go to the two C entry points directly, with every argument prepared: the Python
    # wrappers (ops.stft allocates its output, ops.stft_batch validates and looks its plan up) cost as much
    # host time per call as either kernel runs, and a back-to-back loop through them times the host.
    from danet_amd import _lib
    core, prep, st = _lib.load(), _lib.load_prep(), _lib.stream()
    plan, real_new, real_old = ops._prep_plan(window, N), torch.view_as_real(out), torch.view_as_real(ref)
    a_new = (st, n_utt, pool.data_ptr(), pool.numel(), desc.data_ptr(), T, 0, T, N, S, window.data_ptr(),
             plan.data_ptr(), real_new.data_ptr(), N // 2 + 1)
    a_old = (st, n_utt, Ls, N, S, x.data_ptr(), window.data_ptr(), real_old.data_ptr())

    def new():
        assert prep.danet_prep_stft_batch(*a_new) == 0

    def old():
        assert core.danet_stft(*a_old) == 0
    err = float((got - ref).abs().max() / ref.abs().max())
    del got
    for _ in range(20):
        new()
        old()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(_timed_launches(new, reps))
        t_old.append(_timed_launches(old, reps))
    r = dict(n_utt=n_utt, samples=Ls, N=N, S=S, frames=T, unit='us per launch, C entry points called directly',
             max_rel_diff=err,
             stft_batch=_summary(t_new), danet_stft=_summary(t_old))
    r['ratio_new_over_old'] = round(r['stft_batch']['median'] / r['danet_stft']['median'], 4)
    # the bar: not slower than danet_stft in the same run; a difference inside the block-to-block spread is equal
    r['bar_met'] = bool(r['stft_batch']['median'] <= r['danet_stft']['median'] +
                        max(r['stft_batch']['spread'], r['danet_stft']['spread']))
    print('%d x %d, N %d / S %d: stft_batch %.2f us (spread %.2f), danet_stft %.2f us (spread %.2f), bar_met %s'
          % (n_utt, Ls, N, S, r['stft_batch']['median'], r['stft_batch']['spread'], r['danet_stft']['median'],
             r['danet_stft']['spread'], r['bar_met']), file=sys.stderr)
    return r


def write_tree(root, n_files, seed=0):
    import numpy as np
    import scipy.io.wavfile
    from danet_amd import datasets
    rng = np.random.RandomState(seed)
    for subset, n in (('train', n_files), ('test', 64)):
        os.makedirs(os.path.join(root, subset))
        for i in range(n):
            w = datasets.speech_shaped_wave(rng, int(rng.uniform(1.1, 2.5) * 8000), 8000,
                                            phase=rng.uniform(0, 2 * np.pi))
            scipy.io.wavfile.write(os.path.join(root, subset, 'u%04d.wav' % i), 8000,
                                   np.clip(w, -32768, 32767).astype(np.int16))


def old_route_epoch(ds, batch_size):
    '''the batches of ds.epoch('train') built the way synth-varlen builds variable-length batches'''
    import numpy as np
    import torch
    from danet_amd import utils
    for idx in ds.plan_indices('train', batch_size, shuffle=True):
        waves = [ds.pool_host['train'][ds.offsets['train'][i]:ds.offsets['train'][i] + ds.lengths['train'][i]]
                 for i in idx]
        data = [utils.stft(torch.as_tensor(w)).cpu().numpy() for w in waves]
        max_len = max(map(len, data))
        yield (np.stack([utils.random_zeropad(x, max_len - len(x), axis=-2) for x in data]),)


def feed_row(ds, rounds, epochs):
    import torch
    from danet_amd import feed
    from danet_amd.hparams import hparams
    bs = hparams.BATCH_SIZE * hparams.MAX_N_SIGNAL

    def run(fast):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            src = ds.epoch_device('train', bs, True, 'cuda', hparams.MAX_TRAIN_LEN) if fast else \
                feed.BatchFeed(old_route_epoch(ds, bs), 'cuda', hparams.MAX_TRAIN_LEN)
            for _batch in src:
                n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    run(True)
    run(False)
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(run(True))
        t_old.append(run(False))
    return dict(batch=bs, crop_frames=hparams.MAX_TRAIN_LEN, unit='ms per batch, host clock, no consumer',
                epoch_device=_summary(t_new), per_utterance_stft_batchfeed=_summary(t_old))


def train_row(ds, rounds, epochs):
    import torch
    from danet_amd import cli, datasets, feed
    from danet_amd.hparams import hparams
    from danet_amd.model import Model
    bs = hparams.BATCH_SIZE * hparams.MAX_N_SIGNAL
    model = Model('prep-bench', device='cuda', seed=1337).build()
    model.set_learn_rate(1e-4)
    synth = datasets.SynthSpeechData()
    synth.install_and_load()

    def run(d):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            _rep, k = cli.train_epoch(model, feed.EpochSource(d, 'train', bs, shuffle=True), io.StringIO())
            n += k
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    run(ds)
    run(synth)
    t_w, t_s = [], []
    for _ in range(rounds):
        t_w.append(run(ds))
        t_s.append(run(synth))
    model.check_status()
    return dict(unit='ms per train step incl. the feed, host clock', wavdir=_summary(t_w), synth=_summary(t_s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--out', help='also write the JSON line to this file')
    ap.add_argument('--kernels-only', action='store_true',
                    help='rows (a) and (b) only, nothing written to profiles/ (for a profiler run)')
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.load_package()
    import bench
    from danet_amd import datasets
    from danet_amd.hparams import hparams
    assert torch.cuda.is_available(), 'bench_prep.py measures on the GPU'
    torch.cuda.set_device(0)
    res = dict(workload='wavdir front-end: ragged-batch STFT kernel vs danet_stft, feed and train epoch; '
                        'interleaved blocks in one process', rounds=args.rounds, reps=args.reps,
               device=torch.cuda.get_device_name(0))
    res['a_64x8128_n256_s64'] = kernel_row(64, 8128, 256, 64, args.rounds, args.reps)
    res['b_1x160000_n512_s128'] = kernel_row(1, 160000, 512, 128, args.rounds, args.reps)
    if args.kernels_only:
        print(json.dumps(res))
        return
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'tree')
        write_tree(root, args.files)
        cfg = bench.CONFIGS['cfg2']
        hparams.reset()
        hparams.load(dict(cfg['hp'], BATCH_SIZE=cfg['batch'], NUM_LSTM_LAYERS=cfg['layers'], LSTM_HDIM=cfg['hdim'],
                          MAX_TRAIN_LEN=cfg['frames'], ENCODER_TYPE='bilstm-orig', OPTIMIZER_TYPE='adam',
                          DATASET_TYPE='wavdir', DATASET_DIR=root))
        hparams.digest()
        ds = datasets.WavDirData()
        ds.load_host(out=sys.stderr)
        ds.is_loaded = True
        res['c_feed_64_varlen'] = feed_row(ds, args.rounds, args.epochs)
        res['d_train_epoch_cfg2'] = train_row(ds, args.rounds, args.epochs)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'prep_bench.json'), 'w') as f:
        f.write(line + '\n')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
