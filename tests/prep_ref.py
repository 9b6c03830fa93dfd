'''
Restatement of the ragged-batch STFT of the wavdir dataset (include/danet_prep_hip.h) in float64 numpy /
scipy, and of the dataset's batching plan and draw order -- written from the reference
(app/utils.py:78-122, app/datasets/wsj0.py:40-56, main.py:417-426), independently of datasets.py.
'''
import random

import numpy as np
import scipy.signal


def stft_ref(x, window, N, S):
    '''the reference's call (app/utils.py:117-122) on a float64 copy of x -> complex128 [T, F]'''
    Z = scipy.signal.stft(np.asarray(x, dtype=np.float64), window=np.asarray(window), nperseg=N,
                          noverlap=N - S)[2]
    return Z.T


def num_frames(Ls, N, S):
    '''frames scipy makes of Ls samples (boundary='zeros', padded=True)'''
    ext = Ls + 2 * (N // 2)
    nadd = (-(ext - N) % S) % N
    return (ext + nadd - N) // S + 1


def batch_ref(waves, pads, T_out, window, N, S, t_begin=0, t_count=None):
    '''per utterance the reference's STFT, placed at pad_left on a T_out axis of zeros, then the crop
    -> complex128 [n_utt, t_count, F]'''
    F = N // 2 + 1
    out = np.zeros((len(waves), T_out, F), dtype=np.complex128)
    for u, (w, p) in enumerate(zip(waves, pads)):
        X = stft_ref(w, window, N, S)
        assert p >= 0 and p + len(X) <= T_out
        out[u, p:p + len(X)] = X
    if t_count is None:
        t_count = T_out - t_begin
    return out[:, t_begin:t_begin + t_count]


def index_plan(n, batch_size, shuffle):
    '''app/datasets/wsj0.py:42-47 (np.random when shuffle) -> [n_batch, batch_size]'''
    indices = np.arange(((n + batch_size - 1) // batch_size) * batch_size)
    indices %= n
    if shuffle:
        np.random.shuffle(indices)
    return indices.reshape(-1, batch_size)


def draw_pads(frames):
    '''left pads of one batch, drawn as app/utils.py:78-92 draws them, in utterance order'''
    T_max = max(frames)
    pads = []
    for t in frames:
        padlen = T_max - t
        pads.append(0 if padlen == 0 else random.randint(0, padlen))
    return T_max, pads


def draw_crop(T_max, crop_len):
    '''main.py:422-426 -> (t_begin, t_count)'''
    if crop_len is not None and T_max > crop_len:
        return random.randint(0, T_max - crop_len - 1), crop_len
    return 0, T_max


def bits(a):
    '''complex64 / float32 array -> its uint32 words (bitwise comparisons)'''
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def write_tree(root, seed=0, n_per_subset=40, subsets=('train', 'valid', 'test'), rates=(8000, 11025),
               seconds=(0.6, 1.3)):
    '''a generated wavdir tree of int16 files of speech-shaped noise -> {subset: [paths]}'''
    import os
    import scipy.io.wavfile
    from danet_amd import datasets
    rng = np.random.RandomState(seed)
    made = {}
    for subset in subsets:
        made[subset] = []
        for i in range(n_per_subset):
            rate = rates[i % len(rates)]
            n = int(rng.uniform(*seconds) * rate)
            w = datasets.speech_shaped_wave(rng, n, rate, phase=rng.uniform(0, 2 * np.pi))
            d = os.path.join(str(root), subset, 'spk%d' % (i % 3))
            os.makedirs(d, exist_ok=True)
            fn = os.path.join(d, 'utt%03d.wav' % i)
            scipy.io.wavfile.write(fn, rate, np.clip(w, -32768, 32767).astype(np.int16))
            made[subset].append(fn)
    return made
