'''
Datasets.  Only the reference's data-free `toy` generator
(app/datasets/dataset.py:43-63) is re-stated; `timit` / `wsj0` need licensed
corpora and are out of scope.  `synth` is the speech-shaped 8 kHz
2-speaker generator the benchmarks use.  `wavdir` trains on a folder of the user's
own WAV files: waveforms resident in device memory, every batch one launch of the ragged-batch
STFT kernel (include/danet_prep_hip.h), -- with MIX_SNR_RANGE / MIX_LEVEL_RANGE set -- one launch that
applies the drawn per-utterance gains (include/danet_mix_hip.h), -- with SPEED_PERTURB_RANGE set -- one
launch in front of the STFT that resamples every train utterance by its drawn speed (include/danet_speed_hip.h)
and -- with REVERB_RT60_MAX set -- one launch behind that one that convolves every train utterance with its drawn
room response (include/danet_reverb_hip.h).  With NOISE_DIR set every train batch carries one more STFT launch over
a pool of noise recordings, and the model's front-end adds that noise to the mixture at a drawn SNR while the
targets stay clean (include/danet_noise_hip.h).
'''
import collections
import math
import os
import random
from math import ceil

import numpy as np

from .hparams import hparams


class Dataset(object):
    '''base class (app/datasets/dataset.py:12-35)'''
    def __init__(self):
        self.is_loaded = False

    def epoch(self, subset, batch_size, shuffle=False):
        '''yields (numpy batch [batch_size, T, F],) per batch -- or (that, noise [batch_size / MAX_N_SIGNAL, T, F]):
        a second element is a component of every mixture that is not a target (feed.BatchFeed carries it through as
        a feed.NoisyBatch; only wavdir with NOISE_DIR set yields one).  Two OPTIONAL, independent extensions, both
        looked up by cli through feed.EpochSource: an epoch() that computes its batches on a GPU may take a
        further keyword `device=None` (it is then handed the model's device); a dataset that can build
        the cropped batch on the device offers
        `epoch_device(subset, batch_size, shuffle=False, device=None, crop_len=None)`.'''
        raise NotImplementedError()

    def install_and_load(self):
        raise NotImplementedError()


@hparams.register_dataset('toy')
class WhiteNoiseData(Dataset):
    '''always generates uniform noise rand(batch, 128, FEATURE_SIZE), 10 batches
    per epoch (app/datasets/dataset.py:43-63)'''
    def epoch(self, subset, batch_size, shuffle=False):
        if not self.is_loaded:
            raise RuntimeError('Dataset is not loaded.')
        for _ in range(10):
            signal = np.random.rand(
                batch_size, 128, hparams.FEATURE_SIZE).astype(hparams.FLOATX)
            yield (signal,)

    def install_and_load(self):
        self.is_loaded = True
        return


def speech_shaped_wave(rng, n_samples, smprate=8000, rms=1000.0, phase=0.0):
    '''white N(0,1) -> one-pole low-pass (0.95) -> 3 Hz amplitude envelope ->
    int16-like RMS; the reference feeds un-normalised int16-scale waveforms
    (app/datasets/TIMIT/process.py:44-46)'''
    import scipy.signal
    x = rng.randn(n_samples).astype(np.float32)
    y = scipy.signal.lfilter([1.0], [1.0, -0.95], x)
    t = np.arange(n_samples) / float(smprate)
    y = y * (0.5 * (1.0 + np.sin(2 * np.pi * 3.0 * t + phase)))
    y = y * (rms / (np.sqrt(np.mean(y ** 2)) + 1e-12))
    return y.astype(np.float32)


def synth_waves(seed, n_utt, n_frames, smprate=None):
    '''[n_utt, Ls] float32 waveforms whose STFT has exactly `n_frames` frames
    (T = 1 + ceil(Ls/S))'''
    rng = np.random.RandomState(seed)
    S = hparams.FFT_STRIDE
    Ls = (n_frames - 1) * S
    smprate = smprate or hparams.SMPRATE
    return np.stack([
        speech_shaped_wave(rng, Ls, smprate, phase=rng.uniform(0, 2 * np.pi))
        for _ in range(n_utt)])


@hparams.register_dataset('synth')
class SynthSpeechData(Dataset):
    '''speech-shaped synthetic 2..C-speaker data (SURVEY 8d cfg 2/3): yields
    complex64 spectra [batch, T, FEATURE_SIZE] of independent single-speaker
    utterances, like the reference's TIMIT / WSJ0 iterators
    (app/datasets/timit.py, wsj0.py); mixing happens in the model (main.py:233).
    The STFT runs on the GPU (danet_stft).'''
    N_BATCH = {'train': 10, 'valid': 2, 'test': 2}
    N_FRAMES = 160

    def epoch(self, subset, batch_size, shuffle=False):
        if not self.is_loaded:
            raise RuntimeError('Dataset is not loaded.')
        import torch
        from . import utils
        base = {'train': 0, 'valid': 10 ** 6, 'test': 2 * 10 ** 6}[subset]
        for i in range(self.N_BATCH[subset]):
            seed = base + i if not shuffle else base + int(np.random.randint(0, 10 ** 5))
            waves = synth_waves(seed, batch_size, self.N_FRAMES)
            yield (utils.stft(torch.as_tensor(waves)).cpu().numpy(),)

    def install_and_load(self):
        self.is_loaded = True


@hparams.register_dataset('synth-varlen')
class SynthVarLenSpeechData(SynthSpeechData):
    '''the same generator with utterances of DIFFERENT lengths, batched the way the
    reference's WSJ0 / TIMIT iterators batch variable-length utterances
    (app/datasets/wsj0.py:51-55, timit.py): every spectrogram is zero-padded on both sides
    of the time axis to the longest of the batch by `utils.random_zeropad` (python
    `random`, app/utils.py:78-92).  Padded frames are exact zeros, so a mixture whose
    sources are all padded at a frame has |mix| = 0 there: the argmax / threshold /
    weighted-mean tie cases of the estimators reach the full model.'''
    MIN_FRAMES = 96

    def epoch(self, subset, batch_size, shuffle=False):
        if not self.is_loaded:
            raise RuntimeError('Dataset is not loaded.')
        import torch
        from . import utils
        base = {'train': 0, 'valid': 10 ** 6, 'test': 2 * 10 ** 6}[subset]
        for i in range(self.N_BATCH[subset]):
            seed = base + i if not shuffle else base + int(np.random.randint(0, 10 ** 5))
            rng = np.random.RandomState(seed + 7)
            lens = rng.randint(self.MIN_FRAMES, self.N_FRAMES + 1, size=batch_size)
            waves = synth_waves(seed, batch_size, self.N_FRAMES)
            S = hparams.FFT_STRIDE
            data = [utils.stft(torch.as_tensor(w[:(n - 1) * S])).cpu().numpy()
                    for w, n in zip(waves, lens)]
            max_len = max(map(len, data))
            spectra_li = [utils.random_zeropad(x, max_len - len(x), axis=-2) for x in data]
            yield (np.stack(spectra_li),)


def _stft_frames(n_samples, fft_size, fft_stride):
    '''frames of scipy.signal.stft(boundary='zeros', padded=True) = danet_prep_num_frames'''
    nadd = (-n_samples % fft_stride) % fft_size
    return (n_samples + nadd) // fft_stride + 1


class _DescSlot(object):
    '''one pinned descriptor table (with mixing gains: followed by one float32 per utterance) + its device
    copy + the event behind the last upload out of it'''
    __slots__ = ('pin', 'dev', 'event', 'used')


# the noise of one train batch (WavDirData.plan_noise): per mixture the row into the noise pool (offsets, lengths,
# pads: a danet_prep_utt_t row), the float32 gain, the float64 it was rounded from, the file and the SNR drawn
NoisePlan = collections.namedtuple('NoisePlan', 'offsets lengths pads gains gains64 files snr')


@hparams.register_dataset('wavdir')
class WavDirData(Dataset):
    '''a folder of single-channel WAV files: hparams.DATASET_DIR/{train,valid,test}/**/*.wav, taken in
    sorted path order (a missing `valid` folder falls back to `test`, as app/datasets/timit.py:111-113).

    Files are decoded once (scipy.io.wavfile, float32 at their STORED scale: the reference feeds
    un-normalised int16-scale waveforms), resampled to SMPRATE exactly as utils.load_wavfile does, and
    kept as ONE float32 pool per subset that is uploaded to the device once.  Files shorter than
    FFT_SIZE samples after resampling are skipped and counted.

    Batching is the reference's (app/datasets/wsj0.py:40-56): indices arange(ceil(n/bs)*bs) % n,
    np.random.shuffle when `shuffle`; per batch every spectrogram is zero-padded on both sides of the
    time axis to the longest of the batch, the left pad drawn as utils.random_zeropad draws it.  The
    padded batch is not built on the host: ops.stft_batch writes it in one launch.

    epoch()         the host-literal form every dataset has: numpy complex64 [batch, T_max, F]
    epoch_device()  the fast form: device tensors [B, C, T', F], crop included, no host copy

    MIXTURE LEVELS (hparams.MIX_SNR_RANGE = R, hparams.MIX_LEVEL_RANGE = L, dB, both default None = off: no
    launch, no allocation, no draw, libdanet_mix_hip.so not mapped).  The STFT is linear, so a gain on a
    waveform is a gain on its spectrum: every utterance's mean power is measured once per pool on the device
    (ops.mix_power), every batch draws its gains on the host by the rule include/danet_mix_hip.h writes out
    (plan_gains: sources of a group equalised to their geometric-mean power and offset against each other by
    at most R; the group shifted by one draw from U(-L, L)) and ONE more launch applies them to the batch the
    STFT kernel wrote (ops.mix_scale_); the gains ride in the pinned ring behind the descriptor table.  Draws
    come from a RandomState of the dataset's own per subset, seeded by (dist.shard_seed(1337), subset index):
    `train` runs on across epochs, `valid` / `test` are re-seeded at the start of every sweep.

    SPEED PERTURBATION (hparams.SPEED_PERTURB_RANGE = P, 0 <= P <= 0.25, default None = off: no launch, no
    allocation, no draw, libdanet_speed_hip.so not mapped).  `train` only: every utterance of every train batch
    draws a speed p / 512 (plan_speed, the rule include/danet_speed_hip.h writes out) from a third RandomState,
    seeded by (dist.shard_seed(1337), subset index, 1), BEFORE the batch's pads and crop are planned; the plan
    then sees the new lengths L'.  ONE more launch (ops.speed_resample) writes the resampled batch from the
    resident pool into one of DESC_DEPTH scratch waveform buffers (utterance u at u * stride, stride the longest
    possible L' of the subset rounded up to a multiple of 4), and the STFT kernel reads that scratch; the speed
    descriptors ride in the pinned ring between the STFT descriptors and the gains.  With MIX_SNR_RANGE the
    powers stay those of the stored files.

    REVERBERATION (hparams.REVERB_RT60_MAX = R seconds, 0 <= R <= 1.0, default None = off: no launch, no
    allocation, no draw, libdanet_reverb_hip.so not mapped).  `train` only: every utterance of every train batch
    draws a row of a bank of 32 synthetic room responses (plan_reverb, the rule include/danet_reverb_hip.h writes
    out; row 0 is dry) from a fourth RandomState, seeded by (dist.shard_seed(1337), subset index, 2).  The bank
    is a property of (R, SMPRATE), the same on every rank, and is uploaded once.  ONE more launch
    (ops.reverb_apply) convolves the batch -- from the pool, or from the speed scratch when speed is on too --
    into one of DESC_DEPTH scratch waveform buffers of its own (filled with NaN once, when they are allocated),
    and the STFT kernel reads that scratch.  The tail beyond an utterance's length is cut, so lengths, frames,
    pads and crop are those without the key; the training targets are the reverberant sources.  epoch() asks for
    whole utterances, epoch_device() only for the samples the cropped frames read (reverb_span); the kernel's
    values do not depend on the span, so both routes give the same batches bit for bit.  The 48-byte reverb
    descriptors ride in the pinned ring behind the speed descriptors and before the gains.  With MIX_SNR_RANGE
    the powers stay those of the stored files.

    ADDITIVE NOISE (hparams.NOISE_DIR = a folder of noise recordings, NOISE_SNR_MIN = lo, NOISE_SNR_MAX = hi, dB,
    -30 <= lo <= hi <= 60; all three default None = off: no launch, no allocation, no draw, libdanet_noise_hip.so not
    mapped).  `train` only; `valid` / `test` batches are those without the keys, bit for bit (their noise has keys of
    its own: NOISY EVALUATION below).  NOISE_DIR/**/*.wav is discovered and decoded like the
    dataset's own files into ONE more pool (files shorter than FFT_SIZE skipped and counted).  After a train batch
    is planned as without the keys, plan_noise (the rule include/danet_noise_hip.h writes out) draws per MIXTURE a
    noise file, a position and an SNR from a fifth RandomState, seeded by (dist.shard_seed(1337), subset index, 3):
    a segment of (T_max - 1) * FFT_STRIDE samples of a long file, or a short file whole, placed like a short
    utterance; the gain sets the drawn SNR against the sum of the sources' stored whole-file powers times their
    squared mix gains (so libdanet_mix_hip.so is mapped for its two power launches even with the MIX_* keys null).
    The noise is NOT a row of the batch: ONE more ops.stft_batch launch over the noise pool writes it into a ring of
    OUT_DEPTH buffers of its own, epoch_device() yields feed.NoisyBatch(src, noise, gains), and Model.train_step
    hands the three to ops.noise_frontend in place of ops.frontend -- the targets stay the clean sources.  The
    24-byte noise descriptors and the gains ride in the pinned ring behind the mix gains.  epoch() yields
    (spectra, noise) with the noise already scaled (ops.mix_scale_: the same single rounding), so both routes give
    the same mixture bit for bit.

    NOISY EVALUATION (hparams.NOISE_EVAL_DIR = a folder of held-out noise recordings, NOISE_EVAL_SNR_MIN = lo,
    NOISE_EVAL_SNR_MAX = hi, dB, -30 <= lo <= hi <= 60; all three default None = off: `valid` / `test` are what they
    are without the keys, bit for bit, no launch, no allocation, no draw).  Independent of the three train keys: either
    family works without the other and the two folders may be the same path.  A second pool with its own file,
    offset, length and power tables, read by load_host only when the key is set, uploaded and measured
    (ops.mix_power) at the first noisy evaluation batch.  A `valid` / `test` batch is planned as without the keys;
    then plan_noise, unchanged, runs on the eval tables and bounds with a stream seeded (dist.shard_seed(1337), subset
    index, 4) that is created anew at the start of every sweep (noise_eval_stream): every evaluation sees the same
    noisy mixtures.  `train` never uses this stream or this pool, and `random`, `np.random` and the mix / speed /
    reverb / train-noise streams advance exactly as without the keys.  Both routes carry the noise as for `train`:
    epoch() yields (spectra, noise) with the noise already scaled, epoch_device() yields feed.NoisyBatch(src, noise,
    gains) from one more ops.stft_batch launch into the noise ring, and cli.evaluate hands the three to
    Model.valid_step (include/danet_neval_hip.h: the metric whose baseline is that noisy mixture).

    ACTIVE SPEECH LEVEL (hparams.MIX_LEVEL_MEASURE = "active", default None = mean power: no launch, no allocation,
    libdanet_level_hip.so not mapped, every batch bit for bit what it is without the key).  Needs MIX_SNR_RANGE,
    NOISE_DIR or NOISE_EVAL_DIR: MIX_LEVEL_RANGE alone uses no power.  `train`, `valid` and `test` alike: when a subset's power table
    is measured -- once per pool, an aliased `valid` sharing `test`'s -- ops.mix_power is followed by ONE pass of
    ops.level_activity over the same pool (in launches of rows of similar length whose workspace stays under
    LEVEL_WS_BYTES: level_chunks), and the table holds every file's ITU-T P.56 active power A_c (the rule
    include/danet_level_hip.h writes out: the two-stage envelope against 16 thresholds anchored on the file's own
    rms, 200 ms of hangover, the 15.9 dB margin, finished on the host by active_power) in place of its mean power
    P_c.  Everything that reads the table
    -- G and sqrt(G / P_c) of plan_gains, P_s = sum g_c^2 P_c of plan_noise -- then works on active levels.  The
    noise file's own P_n stays its mean power over its whole length: noise has no pauses to exclude.  With speed
    or reverb on, the level stays that of the stored file, as P_c does.  No draw is added or moved.'''
    SUBSETS = ('train', 'valid', 'test')
    DESC_DEPTH = 8        # pinned descriptor tables in flight
    OUT_DEPTH = 3         # output buffers: a yielded batch stays valid while the next two are drawn

    def __init__(self):
        Dataset.__init__(self)
        self.files, self.lengths, self.offsets, self.frames = {}, {}, {}, {}
        self.pool_host, self.skipped = {}, {}
        self._pool_dev, self._window, self._ring = {}, {}, {}
        self.mix_snr_range = self.mix_level_range = None      # read from hparams by load_host
        self.power = {}             # subset -> float64 mean power sum(x^2) / len of every utterance
        self._mix_rng = {}
        self.speed_range = None     # read from hparams by load_host
        self._speed_rng, self._speed_table, self._speed_scratch = {}, {}, {}
        self.reverb_rt60 = None     # read from hparams by load_host
        self._reverb_rng, self._reverb_bank, self._reverb_scratch = {}, {}, {}
        self.noise_dir = self.noise_snr = None      # read from hparams by load_host: folder, (lo, hi)
        self.noise_files, self.noise_lengths, self.noise_offsets = [], None, None
        self.noise_pool_host, self.noise_skipped, self.noise_power = None, 0, None
        self._noise_rng, self._noise_pool_dev = {}, {}
        # the held-out pool of `valid` / `test` (NOISE_EVAL_*): the same tables a second time
        self.noise_eval_dir = self.noise_eval_snr = None
        self.noise_eval_files, self.noise_eval_lengths, self.noise_eval_offsets = [], None, None
        self.noise_eval_pool_host, self.noise_eval_skipped, self.noise_eval_power = None, 0, None
        self._noise_eval_pool_dev = {}
        self.level_key = None       # read from hparams by load_host: None (mean power) or 'active'
        self._alias = False

    # ---- host half -------------------------------------------------------------------------------
    @staticmethod
    def read_wave(filename):
        '''WAV -> float32 waveform at SMPRATE (utils.load_wavfile up to the STFT)'''
        import scipy.io.wavfile
        import scipy.signal
        smprate, data = scipy.io.wavfile.read(filename)
        if data.ndim != 1:
            raise ValueError('%s has %d channels; the wavdir dataset takes single-channel files'
                             % (filename, data.shape[1]))
        if smprate != hparams.SMPRATE:
            data = scipy.signal.resample(data, int(ceil(len(data) * hparams.SMPRATE / smprate)))
        return np.asarray(data, dtype=np.float32)

    @staticmethod
    def discover(folder):
        '''every *.wav below `folder`, sorted by path'''
        found = []
        for base, _dirs, names in os.walk(folder):
            found += [os.path.join(base, n) for n in names if n.lower().endswith('.wav')]
        return sorted(found)

    @staticmethod
    def mix_ranges():
        '''(MIX_SNR_RANGE, MIX_LEVEL_RANGE) as floats or None; anything but null or a finite number >= 0 is a
        ValueError that names the key'''
        out = []
        for key in ('MIX_SNR_RANGE', 'MIX_LEVEL_RANGE'):
            v = getattr(hparams, key, None)
            if v is not None:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < float('inf'):
                    raise ValueError('hparams.%s must be null or a number of dB >= 0, got %r' % (key, v))
                v = float(v)
            out.append(v)
        return tuple(out)

    @property
    def mix_on(self):
        return self.mix_snr_range is not None or self.mix_level_range is not None

    @staticmethod
    def speed_perturb_range():
        '''SPEED_PERTURB_RANGE as a float or None; anything but null or a number in [0, 0.25] is a ValueError
        that names the key'''
        v = getattr(hparams, 'SPEED_PERTURB_RANGE', None)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 0.25:
                raise ValueError('hparams.SPEED_PERTURB_RANGE must be null or a number in [0, 0.25], got %r' % (v,))
            v = float(v)
        return v

    @staticmethod
    def reverb_rt60_max():
        '''REVERB_RT60_MAX as a float or None; anything but null or a number of seconds in [0, 1.0] is a
        ValueError that names the key, and so is one whose tap count at SMPRATE exceeds the header's envelope'''
        v = getattr(hparams, 'REVERB_RT60_MAX', None)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1.0:
                raise ValueError('hparams.REVERB_RT60_MAX must be null or a number of seconds in [0, 1.0], got %r'
                                 % (v,))
            v = float(v)
            from . import ops
            K = ops.reverb_taps(v, hparams.SMPRATE)
            if K > ops.REVERB_MAX_TAPS:
                raise ValueError('hparams.REVERB_RT60_MAX = %r at SMPRATE = %r needs a room response of %d taps; '
                                 'include/danet_reverb_hip.h takes at most %d' % (v, hparams.SMPRATE, K,
                                                                                  ops.REVERB_MAX_TAPS))
        return v

    NOISE_SNR_LIMITS = (-30.0, 60.0)

    @staticmethod
    def noise_keys():
        '''(NOISE_DIR, (NOISE_SNR_MIN, NOISE_SNR_MAX)) or (None, None) with all three null; anything else is a
        ValueError that names the offending key: a folder that is not a string, a folder without both bounds (the
        missing bound is named), a bound without the folder (NOISE_DIR is named), a bound that is a bool, not a
        number, outside [-30, 60] dB, or lo > hi'''
        return WavDirData._noise_family('NOISE')

    @staticmethod
    def _noise_family(family):
        '''the rule of noise_keys for the keys <family>_DIR, <family>_SNR_MIN, <family>_SNR_MAX'''
        dkey, keys = family + '_DIR', (family + '_SNR_MIN', family + '_SNR_MAX')
        folder = getattr(hparams, dkey, None)
        raw = [getattr(hparams, k, None) for k in keys]
        if folder is not None and not isinstance(folder, str):
            raise ValueError('hparams.%s must be null or the path of a folder of noise recordings, got %r'
                             % (dkey, folder))
        lo_lim, hi_lim = WavDirData.NOISE_SNR_LIMITS
        vals = []
        for key, v in zip(keys, raw):
            if v is not None:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo_lim <= v <= hi_lim:
                    raise ValueError('hparams.%s must be null or a number of dB in [%g, %g], got %r'
                                     % (key, lo_lim, hi_lim, v))
                v = float(v)
            vals.append(v)
        together = 'additive noise needs %s, %s and %s together' % ((dkey,) + keys)
        if folder is None:
            for key, v in zip(keys, vals):
                if v is not None:
                    raise ValueError('hparams.%s is set but hparams.%s is null: %s' % (key, dkey, together))
            return None, None
        for key, v in zip(keys, vals):
            if v is None:
                raise ValueError('hparams.%s is set but hparams.%s is null: %s' % (dkey, key, together))
        if vals[0] > vals[1]:
            raise ValueError('hparams.%s = %r is above hparams.%s = %r' % (keys[0], vals[0], keys[1], vals[1]))
        return folder, (vals[0], vals[1])

    @staticmethod
    def noise_eval_keys():
        '''(NOISE_EVAL_DIR, (NOISE_EVAL_SNR_MIN, NOISE_EVAL_SNR_MAX)) or (None, None): noise_keys for the held-out
        family, independent of the train family'''
        return WavDirData._noise_family('NOISE_EVAL')

    @property
    def noise_on(self):
        return self.noise_dir is not None

    @property
    def noise_eval_on(self):
        return self.noise_eval_dir is not None

    def noisy(self, subset):
        '''does a batch of `subset` carry a noise component: `train` with NOISE_DIR, `valid` / `test` with
        NOISE_EVAL_DIR'''
        return self.noise_on if subset == 'train' else self.noise_eval_on

    LEVEL_MARGIN_DB = 15.9            # P.56: the active level sits this far above the threshold that defines it
    LEVEL_WS_BYTES = 64 << 20         # workspace of one ops.level_activity launch of power_table

    @staticmethod
    def level_measure():
        '''MIX_LEVEL_MEASURE as None or 'active'; anything else -- a bool, a number, another string -- is a
        ValueError that names the key, and so is 'active' at an SMPRATE whose 30 ms time constant exceeds the 4096
        samples include/danet_level_hip.h states its accuracy for'''
        v = getattr(hparams, 'MIX_LEVEL_MEASURE', None)
        if v is None:
            return None
        if not isinstance(v, str) or v != 'active':
            raise ValueError('hparams.MIX_LEVEL_MEASURE must be null (mean power over the whole file) or "active" '
                             '(ITU-T P.56 active speech level), got %r' % (v,))
        if 0.03 * hparams.SMPRATE > 4096:
            raise ValueError('hparams.MIX_LEVEL_MEASURE = "active" needs 0.03 * SMPRATE <= 4096 samples '
                             '(include/danet_level_hip.h), got SMPRATE = %r' % (hparams.SMPRATE,))
        return v

    @staticmethod
    def level_params(smprate):
        '''(g, I) of the level rule at the sampling rate `smprate`: g = exp(-1 / (0.03 fs)), I = ceil(0.2 fs)'''
        return math.exp(-1.0 / (0.03 * smprate)), int(math.ceil(0.2 * smprate))

    @staticmethod
    def level_thresholds(powers):
        '''float64 [n, 16]: c_j = sqrt(P) * 2^(j - 10) of every file's mean power P'''
        P = np.asarray(powers, dtype=np.float64).reshape(-1)
        return np.sqrt(P)[:, None] * np.ldexp(1.0, np.arange(16) - 10)[None, :]

    @staticmethod
    def active_power(sumsq, lengths, counts, thresholds):
        '''the host finish of the level rule (include/danet_level_hip.h, step 4), numpy float64: sumsq [n] the
        sums of squares, lengths [n], counts [n, 16] the activity counts a_j against thresholds [n, 16] -> the
        active powers [n].  The first j with a_j > 0 and A_j - C_j <= M decides: j = 0 gives A_0, a later j the
        linear interpolation in dB between j - 1 and j; none gives the mean power; a silent file keeps 0'''
        sumsq = np.asarray(sumsq, dtype=np.float64).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
        counts = np.asarray(counts).reshape(len(sumsq), -1)
        thresholds = np.asarray(thresholds, dtype=np.float64).reshape(counts.shape)
        M = WavDirData.LEVEL_MARGIN_DB
        out = np.zeros(len(sumsq), dtype=np.float64)
        for u in range(len(sumsq)):
            if not sumsq[u] > 0.0:
                continue
            out[u] = sumsq[u] / lengths[u]
            a = counts[u].astype(np.float64)
            live = a > 0
            A = 10.0 * np.log10(sumsq[u] / np.where(live, a, 1.0))
            diff = A - 20.0 * np.log10(thresholds[u])
            hit = np.nonzero(live & (diff <= M))[0]
            if not len(hit):
                continue
            j = int(hit[0])
            level = A[0]
            if j > 0:
                if not live[j - 1]:       # (cannot happen with ordered thresholds: a_{j-1} >= a_j)
                    continue
                w = (diff[j - 1] - M) / (diff[j - 1] - diff[j])
                level = A[j - 1] + w * (A[j] - A[j - 1])
            out[u] = 10.0 ** (level / 10.0)
        return out

    def load_noise_eval_host(self, out=None):
        '''discover, decode and resample NOISE_EVAL_DIR into ONE host pool of its own, exactly as load_noise_host
        does NOISE_DIR (the two folders may be the same path: two pools all the same)'''
        folder = self.noise_eval_dir
        if not os.path.isdir(folder):
            raise IOError('wavdir: NOISE_EVAL_DIR folder %s not found' % folder)
        files, waves, skipped = [], [], 0
        for fn in self.discover(folder):
            w = self.read_wave(fn)
            if len(w) < hparams.FFT_SIZE:
                skipped += 1
                continue
            files.append(fn)
            waves.append(w)
        print('wavdir held-out evaluation noise (NOISE_EVAL_DIR): %d files, %d shorter than FFT_SIZE skipped'
              % (len(files), skipped), file=out)
        if not files:
            raise IOError('wavdir: no usable WAV file under NOISE_EVAL_DIR = %s' % folder)
        lens = np.asarray([len(w) for w in waves], dtype=np.int64)
        self.noise_eval_files, self.noise_eval_lengths, self.noise_eval_skipped = files, lens, skipped
        self.noise_eval_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.noise_eval_pool_host = np.concatenate(waves)

    def load_noise_host(self, out=None):
        '''discover, decode and resample NOISE_DIR into ONE host pool, exactly like a subset's own files'''
        folder = self.noise_dir
        if not os.path.isdir(folder):
            raise IOError('wavdir: NOISE_DIR folder %s not found' % folder)
        files, waves, skipped = [], [], 0
        for fn in self.discover(folder):
            w = self.read_wave(fn)
            if len(w) < hparams.FFT_SIZE:
                skipped += 1
                continue
            files.append(fn)
            waves.append(w)
        print('wavdir noise: %d files, %d shorter than FFT_SIZE skipped' % (len(files), skipped), file=out)
        if not files:
            raise IOError('wavdir: no usable WAV file under NOISE_DIR = %s' % folder)
        lens = np.asarray([len(w) for w in waves], dtype=np.int64)
        self.noise_files, self.noise_lengths, self.noise_skipped = files, lens, skipped
        self.noise_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        self.noise_pool_host = np.concatenate(waves)

    def load_host(self, out=None):
        '''discover, decode and resample every subset into host pools (no device involved)'''
        self.mix_snr_range, self.mix_level_range = self.mix_ranges()
        self.speed_range = self.speed_perturb_range()
        self.reverb_rt60 = self.reverb_rt60_max()
        self.noise_dir, self.noise_snr = self.noise_keys()
        self.noise_eval_dir, self.noise_eval_snr = self.noise_eval_keys()
        self.level_key = self.level_measure()
        if (self.level_key is not None and self.mix_snr_range is None and self.noise_dir is None
                and self.noise_eval_dir is None):       # (the eval noise rule uses source powers as the train rule)
            raise ValueError('hparams.MIX_LEVEL_MEASURE = %r would do nothing: no source power is used with both '
                             'MIX_SNR_RANGE and NOISE_DIR null (MIX_LEVEL_RANGE alone shifts a mixture without '
                             'measuring it); set one of the two or leave the key null' % (self.level_key,))
        root = hparams.DATASET_DIR
        if root is None:
            raise ValueError('the wavdir dataset needs hparams.DATASET_DIR: the folder that holds '
                             'train/, test/ and optionally valid/')
        for subset in self.SUBSETS:
            folder = os.path.join(root, subset)
            if not os.path.isdir(folder):
                if subset == 'valid':
                    continue
                raise IOError('wavdir: folder %s not found' % folder)
            files, waves, skipped = [], [], 0
            for fn in self.discover(folder):
                w = self.read_wave(fn)
                if len(w) < hparams.FFT_SIZE:
                    skipped += 1
                    continue
                files.append(fn)
                waves.append(w)
            print('wavdir %s: %d files, %d shorter than FFT_SIZE skipped' % (subset, len(files), skipped),
                  file=out)
            if not files:
                raise IOError('wavdir: no usable WAV file under %s' % folder)
            lens = np.asarray([len(w) for w in waves], dtype=np.int64)
            self.files[subset], self.lengths[subset], self.skipped[subset] = files, lens, skipped
            self.offsets[subset] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            self.frames[subset] = np.asarray(
                [_stft_frames(int(n), hparams.FFT_SIZE, hparams.FFT_STRIDE) for n in lens], dtype=np.int64)
            self.pool_host[subset] = np.concatenate(waves)
        self._alias = 'valid' not in self.files
        if self._alias:                   # app/datasets/timit.py:111-113
            for table in (self.files, self.lengths, self.offsets, self.frames, self.pool_host, self.skipped):
                table['valid'] = table['test']
        if self.noise_on:
            self.load_noise_host(out)
        if self.noise_eval_on:
            self.load_noise_eval_host(out)

    def install_and_load(self):
        self.load_host()
        self.is_loaded = True

    # ---- the batching plan (host, no device) -------------------------------------------------------
    def plan_indices(self, subset, batch_size, shuffle=False):
        '''[n_batch, batch_size] utterance indices of one epoch (app/datasets/wsj0.py:42-47)'''
        n = len(self.lengths[subset])
        indices = np.arange(((n + batch_size - 1) // batch_size) * batch_size)
        indices %= n
        if shuffle:
            np.random.shuffle(indices)
        return indices.reshape(-1, batch_size)

    def plan_batch(self, subset, idx, crop_len=None, crop=False, frames=None):
        '''(T_max, pad_left per utterance, t_begin, t_count) of one batch; draws from python's `random`
        exactly as utils.random_zeropad does per utterance (no draw for a full-length one) and then,
        with crop=True, as feed.to_batch_host does for the crop.  frames: the batch's frame counts when
        they are not the stored files' (speed perturbation)'''
        T = self.frames[subset][idx] if frames is None else frames
        T_max = int(T.max())
        pads = [random.randint(0, T_max - int(t)) if T_max > int(t) else 0 for t in T]
        beg, cnt = 0, T_max
        if crop and crop_len is not None and T_max > crop_len:
            beg = random.randint(0, T_max - crop_len - 1)                 # main.py:424-425
            cnt = crop_len
        return T_max, pads, beg, cnt

    # ---- mixture levels: the gain rule (host, no device; include/danet_mix_hip.h) ----------------------
    @staticmethod
    def plan_gains(powers, rng, n_src, snr_range=None, level_range=None):
        '''float32 gains of one batch: `powers` the mean powers of its rows (groups of n_src consecutive rows),
        `rng` the RandomState the draws come from -- per group the n_src - 1 offsets (snr_range set), then the
        level (level_range set)'''
        P = np.asarray(powers, dtype=np.float64).reshape(-1, n_src)
        B, k = len(P), (n_src - 1 if snr_range is not None else 0)
        lo = np.asarray([-snr_range if c < k else -level_range for c in range(k + (level_range is not None))],
                        dtype=np.float64)
        # ONE call draws the whole batch: numpy fills an array draw by draw in row-major order, each as the scalar
        # rng.uniform(lo, hi) would (lo + (hi - lo) * next double), i.e. group by group: offsets, then level
        x = rng.uniform(np.tile(lo, (B, 1)), np.tile(-lo, (B, 1))) if len(lo) else np.zeros((B, 0))
        u = np.concatenate([np.zeros((B, 1)), x[:, :k]], axis=1)
        d = u - u.sum(axis=1, keepdims=True) / n_src
        level = x[:, k:] if level_range is not None else 0.0
        live = P > 0
        gains = 10.0 ** ((d + level) / 20.0)
        if snr_range is not None:
            safe = np.where(live, P, 1.0)
            G = np.exp(np.log(safe).sum(axis=1, keepdims=True) / np.maximum(live.sum(axis=1, keepdims=True), 1))
            gains = np.sqrt(G / safe) * gains
        return np.where(live, gains, 1.0).reshape(-1).astype(np.float32)

    # ---- speed perturbation: the draw (host, no device; include/danet_speed_hip.h) -------------------------
    @staticmethod
    def plan_speed(lengths, rng, P, fft_size):
        '''(p, L') of one batch, two int64 vectors: ONE rng.uniform call draws u ~ U(-P, P) per utterance,
        p = Q + rint(Q u) clipped to Q -+ floor(Q P), L' = floor((L - 1) Q / p) + 1; an utterance whose L'
        would fall below fft_size keeps p = Q'''
        from . import ops
        Q = ops.SPEED_PHASES
        lengths = np.asarray(lengths, dtype=np.int64)
        k = int(np.floor(Q * P))
        u = rng.uniform(-P, P, size=len(lengths))
        p = np.clip(Q + np.rint(Q * u).astype(np.int64), Q - k, Q + k)
        p[ops.speed_out_len(lengths, p) < fft_size] = Q
        return p, ops.speed_out_len(lengths, p)

    def speed_stream(self, subset):
        '''the RandomState the train speeds are drawn from, created once (None with the key null and for
        `valid` / `test`, which are never perturbed)'''
        if self.speed_range is None or subset != 'train':
            return None
        if subset not in self._speed_rng:
            from . import dist
            self._speed_rng[subset] = np.random.RandomState(
                [dist.shard_seed(1337), self.SUBSETS.index(subset), 1])
        return self._speed_rng[subset]

    # ---- reverberation: the draw and the span (host, no device; include/danet_reverb_hip.h) ---------------
    @staticmethod
    def plan_reverb(n, rng):
        '''the bank rows of one batch of n utterances, an int64 vector: ONE rng.randint(0, NB) call'''
        from . import ops
        return rng.randint(0, ops.REVERB_ROWS, size=n).astype(np.int64)

    def reverb_stream(self, subset):
        '''the RandomState the train rows are drawn from, created once (None with the key null and for
        `valid` / `test`, which are never reverberated)'''
        if self.reverb_rt60 is None or subset != 'train':
            return None
        if subset not in self._reverb_rng:
            from . import dist
            self._reverb_rng[subset] = np.random.RandomState(
                [dist.shard_seed(1337), self.SUBSETS.index(subset), 2])
        return self._reverb_rng[subset]

    @staticmethod
    def reverb_span(lengths, pads, beg, cnt, fft_size, fft_stride):
        '''(out_begin, out_count) per utterance, two int64 vectors: the samples that frames [beg, beg + cnt) of
        the padded batch read.  Utterance u's own frame t sits at pads[u] + t of the batch's axis and reads the
        samples [t S - N / 2, t S + N / 2) (include/danet_prep_hip.h: N / 2 zeros in front of the waveform,
        integer framing); what falls outside [0, length) is the transform's zero padding'''
        N, S = fft_size, fft_stride
        first, count = np.zeros(len(lengths), np.int64), np.zeros(len(lengths), np.int64)
        for u, (L, pad) in enumerate(zip(lengths, pads)):
            L, pad = int(L), int(pad)
            a, b = max(beg - pad, 0), min(beg + cnt - pad, _stft_frames(L, N, S))
            if b > a:
                lo, hi = max(a * S - N // 2, 0), min((b - 1) * S + N // 2, L)
                if hi > lo:
                    first[u], count[u] = lo, hi - lo
        return first, count

    # ---- additive noise: the draw, the segment and the gain (host, no device; include/danet_noise_hip.h) --------
    @staticmethod
    def plan_noise(powers, gains, rng, n_src, noise_offsets, noise_lengths, noise_powers, T_max, lo, hi, fft_size,
                   fft_stride):
        '''the NoisePlan of one batch.  powers: the STORED mean powers of its rows (groups of n_src consecutive rows
        are the mixtures), gains: their float32 mix gains or None (= 1), rng: the RandomState the THREE calls draw
        from, each of size B -- files, positions, SNRs.  noise_offsets / noise_lengths / noise_powers: the noise
        pool's tables.  Gains in float64, rounded once to float32; 0 for a silent file or a silent mixture'''
        P = np.asarray(powers, dtype=np.float64).reshape(-1, n_src)
        B = len(P)
        g = (np.ones_like(P) if gains is None
             else np.asarray(gains, dtype=np.float32).astype(np.float64).reshape(-1, n_src))
        f = rng.randint(0, len(noise_lengths), size=B)
        u = rng.random_sample(B)
        snr = rng.uniform(lo, hi, size=B)
        Lfull = (int(T_max) - 1) * fft_stride
        offsets, lengths, pads = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
        g64 = np.zeros(B, np.float64)
        for b in range(B):
            Ln, off = int(noise_lengths[f[b]]), int(noise_offsets[f[b]])
            if Ln >= Lfull:               # a segment of exactly T_max frames
                start = min(int(u[b] * (Ln - Lfull + 1)), Ln - Lfull)
                offsets[b], lengths[b], pads[b] = off + start, Lfull, 0
            else:                         # the whole file, placed like a short utterance
                room = int(T_max) - _stft_frames(Ln, fft_size, fft_stride)
                offsets[b], lengths[b], pads[b] = off, Ln, min(int(u[b] * (room + 1)), room)
            P_s = 0.0
            for c in range(n_src):
                P_s += float(g[b, c]) * float(g[b, c]) * float(P[b, c])
            P_n = float(noise_powers[f[b]])
            if P_s > 0.0 and P_n > 0.0:
                g64[b] = math.sqrt(P_s / P_n) * 10.0 ** (-float(snr[b]) / 20.0)
        return NoisePlan(offsets, lengths, pads, g64.astype(np.float32), g64, f.astype(np.int64), snr)

    def noise_stream(self, subset):
        '''the RandomState the train noise is drawn from, created once (None with the keys null and for `valid` /
        `test`, which never carry noise)'''
        if not self.noise_on or subset != 'train':
            return None
        if subset not in self._noise_rng:
            from . import dist
            self._noise_rng[subset] = np.random.RandomState(
                [dist.shard_seed(1337), self.SUBSETS.index(subset), 3])
        return self._noise_rng[subset]

    def noise_eval_stream(self, subset):
        '''the RandomState the noise of a `valid` / `test` sweep is drawn from, seeded by (dist.shard_seed(1337),
        subset index, 4) and created ANEW by every call -- the start of a sweep, as mix_stream treats these subsets:
        every evaluation sees the same noisy mixtures, ranks draw differently, and `valid` aliased to `test` still has
        its own subset index.  None with the keys null and for `train`, which never uses this stream or this pool'''
        if not self.noise_eval_on or subset == 'train':
            return None
        from . import dist
        return np.random.RandomState([dist.shard_seed(1337), self.SUBSETS.index(subset), 4])

    def noise_tables(self, subset):
        '''(offsets, lengths, powers, (lo, hi)) of the pool `subset` draws its noise from'''
        if subset == 'train':
            return self.noise_offsets, self.noise_lengths, self.noise_power, self.noise_snr
        return self.noise_eval_offsets, self.noise_eval_lengths, self.noise_eval_power, self.noise_eval_snr

    def _pool_key(self, subset):
        return 'test' if (subset == 'valid' and self._alias) else subset

    def mix_stream(self, subset):
        '''the RandomState `subset`'s gains are drawn from (None with both keys null): the train stream is
        created once, the valid / test streams anew by every call -- the start of a sweep'''
        if not self.mix_on:
            return None
        if subset != 'train' or subset not in self._mix_rng:
            from . import dist
            self._mix_rng[subset] = np.random.RandomState([dist.shard_seed(1337), self.SUBSETS.index(subset)])
        return self._mix_rng[subset]

    def plan_epoch(self, subset, batch_size, shuffle=False, crop_len=None, crop=False):
        '''the host plan of one epoch, per batch (idx, T_max, pads, t_begin, t_count, gains): plan_indices, then
        per batch plan_batch and -- with a MIX_* key set -- plan_gains on self.power (else gains is None and
        nothing is drawn).  `random` / `np.random` advance exactly as without the keys.  With
        SPEED_PERTURB_RANGE set the train plan is the one of the drawn lengths (plan_epoch_speed).'''
        for item in self.plan_epoch_reverb(subset, batch_size, shuffle, crop_len, crop):
            yield item[:6]

    def plan_epoch_speed(self, subset, batch_size, shuffle=False, crop_len=None, crop=False):
        '''plan_epoch with a seventh field: None, or -- `train` with SPEED_PERTURB_RANGE set -- the (p, L') of
        plan_speed, drawn per batch before plan_batch, which then plans the frames of the new lengths'''
        for item in self.plan_epoch_reverb(subset, batch_size, shuffle, crop_len, crop):
            yield item[:7]

    def plan_epoch_reverb(self, subset, batch_size, shuffle=False, crop_len=None, crop=False):
        '''plan_epoch_speed with an eighth field: None, or -- `train` with REVERB_RT60_MAX set -- the bank rows
        of plan_reverb, drawn per batch from a stream of their own (nothing else moves)'''
        rng = self.mix_stream(subset)
        speed_rng = self.speed_stream(subset)
        reverb_rng = self.reverb_stream(subset)
        C = hparams.MAX_N_SIGNAL
        if rng is not None and batch_size % C:
            raise ValueError('wavdir: with MIX_SNR_RANGE / MIX_LEVEL_RANGE set the batch size must be a multiple '
                             'of MAX_N_SIGNAL = %d (got %d): gains are drawn per group of sources' % (C, batch_size))
        for idx in self.plan_indices(subset, batch_size, shuffle):
            speed = frames = None
            if speed_rng is not None:
                speed = self.plan_speed(self.lengths[subset][idx], speed_rng, self.speed_range, hparams.FFT_SIZE)
                frames = np.asarray([_stft_frames(int(n), hparams.FFT_SIZE, hparams.FFT_STRIDE) for n in speed[1]],
                                    dtype=np.int64)
            T_max, pads, beg, cnt = self.plan_batch(subset, idx, crop_len, crop, frames)
            gains = None
            if rng is not None:
                gains = self.plan_gains(self.power[self._pool_key(subset)][idx], rng, C,
                                        self.mix_snr_range, self.mix_level_range)
            rows = self.plan_reverb(len(idx), reverb_rng) if reverb_rng is not None else None
            yield idx, T_max, pads, beg, cnt, gains, speed, rows

    def plan_epoch_noise(self, subset, batch_size, shuffle=False, crop_len=None, crop=False):
        '''plan_epoch_reverb with a ninth field: None, or -- `train` with NOISE_DIR set, `valid` / `test` with
        NOISE_EVAL_DIR set -- the NoisePlan of plan_noise on that subset's pool and bounds (noise_tables), drawn per
        batch AFTER everything else from a stream of its own (nothing else moves).  Needs the power tables
        (self.power, self.noise_power / self.noise_eval_power: the device half measures them)'''
        noise_rng = self.noise_stream(subset) if subset == 'train' else self.noise_eval_stream(subset)
        C = hparams.MAX_N_SIGNAL
        if noise_rng is not None and batch_size % C:
            raise ValueError('wavdir: with %s set the batch size must be a multiple of MAX_N_SIGNAL = %d (got '
                             '%d): noise is drawn per mixture'
                             % ('NOISE_DIR' if subset == 'train' else 'NOISE_EVAL_DIR', C, batch_size))
        if noise_rng is not None:
            offsets, lengths, powers, (lo, hi) = self.noise_tables(subset)
        for item in self.plan_epoch_reverb(subset, batch_size, shuffle, crop_len, crop):
            noise = None
            if noise_rng is not None:
                noise = self.plan_noise(self.power[self._pool_key(subset)][item[0]], item[5], noise_rng, C,
                                        offsets, lengths, powers, item[1], lo, hi, hparams.FFT_SIZE,
                                        hparams.FFT_STRIDE)
            yield item + (noise,)

    # ---- device half -----------------------------------------------------------------------------
    @staticmethod
    def _device(device=None):
        import torch
        device = torch.device('cuda' if device is None else device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        return device

    def upload_pool(self, subset, device):
        '''the subset's float32 pool on `device` (uploaded once)'''
        import torch
        key = (self._pool_key(subset), str(device))
        pool = self._pool_dev.get(key)
        if pool is None:
            pool = self._pool_dev[key] = torch.from_numpy(self.pool_host[subset]).to(device)
        return pool

    def power_table(self, subset, pool):
        '''float64 mean power of every utterance of the subset, measured on the device once (ops.mix_power on
        the uploaded pool; an aliased `valid` shares `test`'s table).  With MIX_LEVEL_MEASURE = "active" the table
        holds the active powers instead (active_table)'''
        key = self._pool_key(subset)
        table = self.power.get(key)
        if table is None:
            from . import ops
            sums = ops.mix_power(pool, self.offsets[subset], self.lengths[subset]).cpu().numpy()
            if self.level_key is not None:
                table = self.power[key] = self.active_table(subset, pool, sums)
                return table
            table = self.power[key] = sums / self.lengths[subset].astype(np.float64)
        return table

    def active_table(self, subset, pool, sums):
        '''float64 active power of every utterance of the subset from its sums of squares: the thresholds of
        its mean power, ops.level_activity over the pool -- in the launches of level_chunks; the counts do not depend
        on how the rows are grouped -- and the host finish'''
        from . import ops
        offsets, lengths = self.offsets[subset], self.lengths[subset]
        g, hang = self.level_params(hparams.SMPRATE)
        thr = self.level_thresholds(sums / lengths.astype(np.float64))
        counts = np.zeros((len(lengths), ops.LEVEL_THRESHOLDS), dtype=np.int64)
        for rows in self.level_chunks(lengths, self.LEVEL_WS_BYTES):
            counts[rows] = ops.level_activity(pool, offsets[rows], lengths[rows], thr[rows], g, hang).cpu().numpy()
        return self.active_power(sums, lengths, counts, thr)

    @staticmethod
    def level_chunks(lengths, ws_bytes):
        '''the rows of a pool in launches of ops.level_activity whose workspace -- rows x tiles of the LONGEST row
        of the launch x 208 bytes -- stays under ws_bytes (one row is always taken): index vectors, longest rows
        first, so that a launch holds rows of similar length'''
        from . import ops
        lengths = np.asarray(lengths, dtype=np.int64)
        order = np.argsort(-lengths, kind='stable')
        a = 0
        while a < len(order):
            tiles = max(1, -(-int(lengths[order[a]]) // ops.LEVEL_TILE))
            step = max(1, int(ws_bytes) // (tiles * (16 + 12 * ops.LEVEL_THRESHOLDS)))
            yield order[a:a + step]
            a += step

    def upload_noise_eval(self, device):
        '''upload_noise for the held-out pool of NOISE_EVAL_DIR: uploaded once, and measured once (ops.mix_power), at
        the first noisy evaluation batch'''
        import torch
        pool = self._noise_eval_pool_dev.get(str(device))
        if pool is None:
            pool = self._noise_eval_pool_dev[str(device)] = torch.from_numpy(self.noise_eval_pool_host).to(device)
        if self.noise_eval_power is None:
            from . import ops
            sums = ops.mix_power(pool, self.noise_eval_offsets, self.noise_eval_lengths).cpu().numpy()
            self.noise_eval_power = sums / self.noise_eval_lengths.astype(np.float64)
        return pool

    def _noise_pool_on(self, device, subset):
        return self.upload_noise(device) if subset == 'train' else self.upload_noise_eval(device)

    def upload_noise(self, device):
        '''the float32 noise pool on `device` (uploaded once) and, measured on it once, every noise file's float64
        mean power over its whole length (ops.mix_power)'''
        import torch
        pool = self._noise_pool_dev.get(str(device))
        if pool is None:
            pool = self._noise_pool_dev[str(device)] = torch.from_numpy(self.noise_pool_host).to(device)
        if self.noise_power is None:
            from . import ops
            sums = ops.mix_power(pool, self.noise_offsets, self.noise_lengths).cpu().numpy()
            self.noise_power = sums / self.noise_lengths.astype(np.float64)
        return pool

    def speed_table_on(self, device):
        '''the filter table of the key's P on `device` (float64 numpy rounded once, uploaded once per dataset)'''
        t = self._speed_table.get(str(device))
        if t is None:
            import torch
            from . import ops
            t = self._speed_table[str(device)] = torch.from_numpy(ops.speed_table(self.speed_range)).to(device)
        return t

    def speed_stride(self, subset):
        '''floats between two utterances of a scratch waveform buffer: the longest L' any draw can give the
        subset's longest file (at most max L / (1 - P) + 1), rounded up to a multiple of 4'''
        from . import ops
        p_min = ops.SPEED_PHASES - int(np.floor(ops.SPEED_PHASES * self.speed_range))
        return (int(ops.speed_out_len(int(self.lengths[subset].max()), p_min)) + 3) & ~3

    def _take_scratch(self, device, subset, n_utt):
        '''the next of DESC_DEPTH scratch waveform buffers of the subset (allocated once; as deep as the
        descriptor ring: batches are built ahead of their consumer) -> (float32 device vector, stride)'''
        import torch
        key = (subset, str(device))
        ring = self._speed_scratch.get(key)
        if ring is None or ring['n_utt'] < n_utt:
            stride = self.speed_stride(subset)
            ring = self._speed_scratch[key] = dict(
                n_utt=n_utt, stride=stride, k=0,
                bufs=[torch.empty(n_utt * stride, dtype=torch.float32, device=device) for _ in range(self.DESC_DEPTH)])
        ring['k'] += 1
        return ring['bufs'][(ring['k'] - 1) % self.DESC_DEPTH], ring['stride']

    def reverb_bank_on(self, device):
        '''the bank of room responses of the key's R on `device` (float64 numpy rounded once, uploaded once per
        dataset) -> float32 [32, K]'''
        t = self._reverb_bank.get(str(device))
        if t is None:
            import torch
            from . import ops
            t = self._reverb_bank[str(device)] = torch.from_numpy(
                ops.reverb_bank(self.reverb_rt60, hparams.SMPRATE)).to(device)
        return t

    def _take_reverb_scratch(self, device, subset, n_utt):
        '''the next of DESC_DEPTH scratch buffers of reverberated waveforms of the subset (allocated once and
        filled with NaN once, so that a frame that reads outside the span asked for is loud) -> (float32 device
        vector, stride: speed's when speed is on, else the subset's longest file rounded up to a multiple of 4)'''
        import torch
        key = (subset, str(device))
        ring = self._reverb_scratch.get(key)
        if ring is None or ring['n_utt'] < n_utt:
            stride = (self.speed_stride(subset) if self.speed_range is not None
                      else (int(self.lengths[subset].max()) + 3) & ~3)
            ring = self._reverb_scratch[key] = dict(
                n_utt=n_utt, stride=stride, k=0,
                bufs=[torch.full((n_utt * stride,), float('nan'), dtype=torch.float32, device=device)
                      for _ in range(self.DESC_DEPTH)])
        ring['k'] += 1
        return ring['bufs'][(ring['k'] - 1) % self.DESC_DEPTH], ring['stride']

    def _window_on(self, device):
        import torch
        w = self._window.get(str(device))
        if w is None:
            w = self._window[str(device)] = torch.as_tensor(
                np.asarray(hparams.FFT_WND, dtype=np.float32)).to(device)
        return w

    def epoch(self, subset, batch_size, shuffle=False, device=None):
        '''numpy complex64 [batch_size, T_max, F] per batch.  The spectra are computed on `device` (default:
        the current CUDA device; cli passes the model's, so the pool is uploaded once, where the model is)'''
        if not self.is_loaded:
            raise RuntimeError('Dataset is not loaded.')
        import torch
        from . import ops
        device = self._device(device)
        pool, window = self.upload_pool(subset, device), self._window_on(device)
        noisy = self.noisy(subset)
        if self.mix_on or noisy:
            self.power_table(subset, pool)
        noise_pool = self._noise_pool_on(device, subset) if noisy else None
        for idx, T_max, pads, _beg, _cnt, gains, speed, rows, noise in self.plan_epoch_noise(subset, batch_size,
                                                                                             shuffle):
            src, offsets, lengths = pool, self.offsets[subset][idx], self.lengths[subset][idx]
            if speed is not None:         # resampled into a scratch buffer the STFT then reads
                src, stride = self._take_scratch(device, subset, batch_size)
                spots = np.arange(len(idx), dtype=np.int64) * stride
                ops.speed_resample(pool, ops.speed_desc(offsets, lengths, spots, speed[1], speed[0], pool.numel(),
                                                        src.numel()), self.speed_table_on(device), src)
                offsets, lengths = spots, speed[1]
            if rows is not None:          # whole utterances convolved into a scratch buffer the STFT then reads
                dry, (src, stride) = src, self._take_reverb_scratch(device, subset, batch_size)
                spots = np.arange(len(idx), dtype=np.int64) * stride
                bank = self.reverb_bank_on(device)
                ops.reverb_apply(dry, ops.reverb_desc(offsets, lengths, spots, np.zeros(len(idx), np.int64), lengths,
                                                      rows, dry.numel(), src.numel()), bank, bank.shape[1], src)
                offsets = spots
            desc = ops.prep_desc(offsets, lengths, pads, T_max, src.numel(), hparams.FFT_SIZE, hparams.FFT_STRIDE)
            spectra = ops.stft_batch(src, desc, T_max, window, hparams.FFT_SIZE, hparams.FFT_STRIDE,
                                     t_begin=0, t_count=T_max)
            if gains is not None:
                ops.mix_scale_(spectra, torch.from_numpy(gains).to(device))
            if noise is not None:         # all T_max frames of the noise, scaled: the single rounding fl(g * n)
                ndesc = ops.prep_desc(noise.offsets, noise.lengths, noise.pads, T_max, noise_pool.numel(),
                                      hparams.FFT_SIZE, hparams.FFT_STRIDE)
                nspec = ops.stft_batch(noise_pool, ndesc, T_max, window, hparams.FFT_SIZE, hparams.FFT_STRIDE,
                                       t_begin=0, t_count=T_max)
                ops.mix_scale_(nspec, torch.from_numpy(noise.gains).to(device))
                yield (spectra.cpu().numpy(), nspec.cpu().numpy())
                continue
            yield (spectra.cpu().numpy(),)

    def _take_ring(self, device, n_utt):
        import torch
        from . import ops
        row = ops.PREP_DESC_DTYPE.itemsize + (4 if self.mix_on else 0)      # + one float32 gain
        if self.speed_range is not None:
            row += ops.SPEED_DESC_DTYPE.itemsize                            # + one speed descriptor
        if self.reverb_rt60 is not None:
            row += ops.REVERB_DESC_DTYPE.itemsize                           # + one reverb descriptor
        if self.noise_on or self.noise_eval_on:
            row += ops.PREP_DESC_DTYPE.itemsize + 4 + 8     # per MIXTURE a noise descriptor and a gain (+ alignment)
        ring = self._ring.get(str(device))
        if ring is None or ring['n_utt'] < n_utt or ring['row'] < row:
            slots = []
            for _ in range(self.DESC_DEPTH):
                s = _DescSlot()
                s.pin = torch.zeros(n_utt * row, dtype=torch.uint8).pin_memory()
                s.dev = torch.zeros(n_utt * row, dtype=torch.uint8, device=device)
                s.event, s.used = torch.cuda.Event(), False
                slots.append(s)
            ring = self._ring[str(device)] = dict(n_utt=n_utt, row=row, slots=slots, out=[None] * self.OUT_DEPTH,
                                                  k=0)
        return ring

    def epoch_device(self, subset, batch_size, shuffle=False, device=None, crop_len=None):
        '''the batches of epoch() -- same index plan, same pad draws -- followed by the crop draw of
        feed.to_batch_host, as complex64 DEVICE tensors [BATCH_SIZE, MAX_N_SIGNAL, T', F]: one
        ops.stft_batch launch per batch computes only the cropped frames; per batch a 24-byte row per
        utterance (28 with mixing gains, followed by their one launch) crosses PCIe, from a pinned ring,
        without a host wait.  Everything is enqueued on the
        stream that is current in the consumer.  LIFETIME: a yielded tensor is a view of one of
        OUT_DEPTH reused device buffers and stays valid until the consumer has asked for OUT_DEPTH - 1
        more batches (the same rule as feed.BatchFeed; clone it to keep it longer).  `train` with NOISE_DIR set, and
        `valid` / `test` with NOISE_EVAL_DIR set: one more launch per batch, and what is yielded is a feed.NoisyBatch(src, noise [B, T', F], gains [B]) whose
        three tensors live by the same rule.'''
        if not self.is_loaded:
            raise RuntimeError('Dataset is not loaded.')
        device = self._device(device)
        F, B, C = hparams.FEATURE_SIZE, hparams.BATCH_SIZE, hparams.MAX_N_SIGNAL
        assert batch_size == B * C, (batch_size, B, C)
        pool, window = self.upload_pool(subset, device), self._window_on(device)
        noisy = self.noisy(subset)
        if self.mix_on or noisy:
            self.power_table(subset, pool)
        if noisy:
            self._noise_pool_on(device, subset)
        ring = self._take_ring(device, batch_size)
        for idx, T_max, pads, beg, cnt, gains, speed, rows, noise in self.plan_epoch_noise(subset, batch_size, shuffle,
                                                                                           crop_len, crop=True):
            more = {}
            if gains is not None:
                more['gains'] = gains
            if speed is not None:
                more['speed'] = speed
            if rows is not None:
                more['reverb'] = rows
            if noise is not None:         # one more launch; the front-end adds the noise (feed.NoisyBatch)
                from . import feed
                out, nout, ngains = self._emit(device, pool, window, ring, subset, idx, T_max, pads, beg, cnt,
                                               noise=noise, **more)
                yield feed.NoisyBatch(out.view(B, C, cnt, F), nout, ngains)
                continue
            out = self._emit(device, pool, window, ring, subset, idx, T_max, pads, beg, cnt, **more)
            yield out.view(B, C, cnt, F)

    def _emit(self, device, pool, window, ring, subset, idx, T_max, pads, beg, cnt, gains=None, speed=None,
              reverb=None, noise=None):
        '''the device half of one batch: descriptor table (and the speed descriptors, the reverb descriptors and
        the gains behind it, in the same copy) through the pinned ring, (one launch that resamples the batch into
        a scratch waveform buffer, one that convolves the samples the cropped frames read into another,) one
        launch into the next output buffer (and one that scales it in place) -> complex64 [batch, cnt, F].
        noise (a NoisePlan): its descriptors and gains ride behind the mix gains in the same copy, and one more STFT
        launch over the noise pool writes the same frames of the noise into the next of OUT_DEPTH noise buffers
        -> (that batch, noise complex64 [mixtures, cnt, F], float32 device gains [mixtures])'''
        import torch
        from . import ops
        N, S, F = hparams.FFT_SIZE, hparams.FFT_STRIDE, hparams.FEATURE_SIZE
        batch_size, row = len(idx), ops.PREP_DESC_DTYPE.itemsize
        k = ring['k']
        ring['k'] = k + 1
        slot = ring['slots'][k % self.DESC_DEPTH]
        if slot.used:
            slot.event.synchronize()      # the copy out of this table DESC_DEPTH batches ago: long done
        table = slot.pin[:batch_size * row].numpy().view(ops.PREP_DESC_DTYPE)
        dev_table, sent = slot.dev[:batch_size * row], batch_size * row
        src, offsets, lengths = pool, self.offsets[subset][idx], self.lengths[subset][idx]
        if speed is not None:             # 40-byte rows right behind the table: the scratch the STFT then reads
            src, stride = self._take_scratch(device, subset, batch_size)
            spots = np.arange(batch_size, dtype=np.int64) * stride
            at, sent = sent, sent + batch_size * ops.SPEED_DESC_DTYPE.itemsize
            ops.speed_desc(offsets, lengths, spots, speed[1], speed[0], pool.numel(), src.numel(),
                           out=slot.pin[at:sent].numpy().view(ops.SPEED_DESC_DTYPE))
            dev_speed, offsets, lengths = slot.dev[at:sent], spots, speed[1]
        if reverb is not None:            # 48-byte rows behind those: the scratch the STFT reads instead
            dry, (src, stride) = src, self._take_reverb_scratch(device, subset, batch_size)
            spots = np.arange(batch_size, dtype=np.int64) * stride
            at, sent = sent, sent + batch_size * ops.REVERB_DESC_DTYPE.itemsize
            first, count = self.reverb_span(lengths, pads, beg, cnt, N, S)
            ops.reverb_desc(offsets, lengths, spots, first, count, reverb, dry.numel(), src.numel(),
                            out=slot.pin[at:sent].numpy().view(ops.REVERB_DESC_DTYPE))
            dev_reverb, offsets = slot.dev[at:sent], spots
        ops.prep_desc(offsets, lengths, pads, T_max, src.numel(), N, S, out=table)
        if gains is not None:             # float32 [batch] behind the descriptors: one copy carries them all
            at, sent = sent, sent + batch_size * 4
            slot.pin[at:sent].numpy().view(np.float32)[:] = gains
            dev_gains = slot.dev[at:sent].view(torch.float32)
        if noise is not None:             # 24-byte rows (8-byte aligned) and float32 [mixtures] behind everything
            noise_pool, n_mix = self._noise_pool_on(device, subset), len(noise.gains)
            at = (sent + 7) & ~7
            sent = at + n_mix * row
            ops.prep_desc(noise.offsets, noise.lengths, noise.pads, T_max, noise_pool.numel(), N, S,
                          out=slot.pin[at:sent].numpy().view(ops.PREP_DESC_DTYPE))
            dev_noise_table = slot.dev[at:sent]
            at, sent = sent, sent + n_mix * 4
            slot.pin[at:sent].numpy().view(np.float32)[:] = noise.gains
            dev_noise_gains = slot.dev[at:sent].view(torch.float32)
        slot.dev[:sent].copy_(slot.pin[:sent], non_blocking=True)
        slot.event.record(torch.cuda.current_stream(device))
        slot.used = True
        n = batch_size * cnt * F
        buf = ring['out'][k % self.OUT_DEPTH]
        if buf is None or buf.numel() < n:
            buf = ring['out'][k % self.OUT_DEPTH] = torch.empty(n, dtype=torch.complex64, device=device)
        out = buf[:n].view(batch_size, cnt, F)
        if speed is not None:
            ops.speed_resample(pool, dev_speed, self.speed_table_on(device), dry if reverb is not None else src)
        if reverb is not None:
            bank = self.reverb_bank_on(device)
            ops.reverb_apply(dry, dev_reverb, bank, bank.shape[1], src)
        ops.stft_batch(src, dev_table, T_max, window, N, S, t_begin=beg, t_count=cnt, out=out)
        if gains is not None:
            ops.mix_scale_(out, dev_gains)
        if noise is not None:
            nring = ring.setdefault('noise_out', [None] * self.OUT_DEPTH)
            n = n_mix * cnt * F
            nbuf = nring[k % self.OUT_DEPTH]
            if nbuf is None or nbuf.numel() < n:
                nbuf = nring[k % self.OUT_DEPTH] = torch.empty(n, dtype=torch.complex64, device=device)
            nout = nbuf[:n].view(n_mix, cnt, F)
            ops.stft_batch(noise_pool, dev_noise_table, T_max, window, N, S, t_begin=beg, t_count=cnt, out=nout)
            return out, nout, dev_noise_gains
        return out
