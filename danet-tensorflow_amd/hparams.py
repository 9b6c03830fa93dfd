'''
Hyperparameter bag + plugin registries.

Mirrors the reference's `app/hparams.py:15-130` surface (same keys as
`default.json:1-41`, same `register_*` / `get_*` names, same `digest()`
derivations) so `hparams.get_encoder()` etc. resolve the MI355X-native plugins
unchanged.  Differences, all deliberate:

* `FFT_WND` is still an expression string; it is evaluated with `np`, `scipy`
  and `self` in scope like the reference (`app/hparams.py:42`), but
  `scipy.signal.hann` (removed from current scipy) is aliased to
  `scipy.signal.windows.hann`.
* Two keys are added with the reference's hard-coded values as defaults
  (`app/modules.py:212,223-242`): `NUM_LSTM_LAYERS=4`, `LSTM_HDIM=300`.
* `DROPOUT_KEEP_PROB` reaches the encoder: the reference feeds it on every train
  step (`main.py:429`) but calls the encoder without it (`main.py:243`); here
  `Model.train_step` passes it on and the BiLSTM encoders apply
  `tf.nn.dropout` where `_lyr_bilstm` has it (`app/modules.py:137`).  The
  default 1.0 is exactly the reference's behaviour.
* `DATASET_DIR` (default None) names the folder the `wavdir` dataset reads.
* `MIX_SNR_RANGE` / `MIX_LEVEL_RANGE` (dB, default None = off) make the `wavdir` dataset mix
  its sources at a drawn relative level / shift the whole mixture by a drawn level
  (the reference's `# TODO add mixing coeff ?`, `main.py:230`); every other dataset ignores them.
* `SPEED_PERTURB_RANGE` (a fraction in [0, 0.25], default None = off) makes the `wavdir` dataset
  resample every utterance of every train batch by a drawn speed factor; every other dataset ignores it.
* `REVERB_RT60_MAX` (seconds in [0, 1.0], default None = off) makes the `wavdir` dataset convolve every
  utterance of every train batch with a drawn synthetic room response; every other dataset ignores it.
* `NOISE_DIR` (a folder of noise recordings) with `NOISE_SNR_MIN` / `NOISE_SNR_MAX` (dB, -30 <= min <= max <= 60;
  all three default None = off) make the `wavdir` dataset add a drawn segment of a drawn noise file to every train
  mixture at a drawn SNR, the targets staying clean; every other dataset ignores them.
* `NOISE_EVAL_DIR` (a folder of held-out noise recordings) with `NOISE_EVAL_SNR_MIN` / `NOISE_EVAL_SNR_MAX` (dB,
  -30 <= min <= max <= 60; all three default None = off) do the same to every `valid` / `test` mixture of the `wavdir`
  dataset, the same noise in every sweep; independent of the `NOISE_*` keys; with `EVAL_SI_SDR` true `Model.valid_step`
  then reports `SI-SDR` / `SI-SDRi` against the noisy mixture and `nSNR`; every other dataset ignores them.
* `MIX_LEVEL_MEASURE` (`"active"`, default None = mean power over the whole file) makes the `wavdir` dataset set
  `MIX_SNR_RANGE` / `NOISE_SNR_*` levels from every source's ITU-T P.56 active speech level, pauses excluded;
  every other dataset ignores it.
* `EVAL_SI_SDR` (true / false, default None = off) makes `Model.valid_step` return `SI-SDR` and `SI-SDRi` of the
  separated waveforms next to `loss` and `SNR`, for every dataset; `train_step` and `infer` never compute it.
* `TRAIN_LOSS` (`"pit-mse"` / `"si-sdr"`, default None = `"pit-mse"`) chooses what `Model.train_step` minimises: the
  reference's PIT-MSE on complex spectra, or minus the SI-SDR (dB) of the separated waveforms; validation is untouched.
* `GRAD_CLIP_NORM` (a finite number > 0, default None = off) makes `Model.train_step` scale the whole gradient so that
  its global L2 norm does not exceed the value (`torch.nn.utils.clip_grad_norm_`'s rule), before the value clip
  `GRAD_CLIP_THRES`; the step then also returns `grad_norm` and `clip_coef`.
* `DPCL_WEIGHT` (a finite number >= 0, default None = off) adds that many times the deep-clustering affinity loss of
  the embedding against the ideal binary mask to what `Model.train_step` minimises; the step then also returns `DPCL`.
* `INFER_CHUNK_LEN` (frames, a multiple of `LENGTH_ALIGN`, >= 2; default None = off) makes `Model.infer` separate a
  recording longer than that in overlapping chunks batched through the encoder and stitch them back together with
  speaker-continuity tracking; `INFER_CHUNK_OVERLAP` (frames of cross-fade, 1 <= V <= L // 2, default None =
  max(1, L // 4)) and `INFER_CHUNK_BATCH` (chunks per encoder launch group, >= 1, default None = 16) need it;
  `train_step`, `valid_step` and `debug_fetch` never look at them.
* `EVAL_BSS_SDR` (true / false, default None = off) makes `Model.valid_step` also return the BSS-eval v3
  (`bss_eval_sources`) figures `SDR`, `SIR`, `SAR` and `SDRi` of the separated waveforms, in dB, for every dataset;
  `EVAL_BSS_FILTER_LEN` (an integer in 1..512, default None = 512) is the length of the allowed distortion filter and
  needs it; not with `NOISE_EVAL_DIR`; `train_step`, `infer` and `debug_fetch` never compute them.
* `EVAL_STOI` (true / false, default None = off) makes `Model.valid_step` also return the intelligibility figures
  `STOI`, `ESTOI` and their improvements over the mixture `STOIi`, `ESTOIi` of the separated waveforms, for every
  dataset; it needs `SMPRATE` >= 8000 with a resampling table to 10 kHz of at most 16384 entries; not with
  `NOISE_EVAL_DIR`; `train_step`, `infer` and `debug_fetch` never compute them.
* `PHASE_REFINE_ITERS` (an integer in 1..100, default None = off) makes `Model.infer` (chunked inference included) and
  the waveform metrics of `Model.valid_step` run that many iterations of MISI phase refinement (multiple-input
  spectrogram inversion) on the separated spectra, which otherwise carry the mixture's phase; `loss` and `SNR` stay
  the figures of the unrefined output; not with `NOISE_EVAL_DIR`; `train_step` and `debug_fetch` never look at it.
* `INFER_ESTIMATOR_METHOD = "online"` selects the online attractor estimator: attractors that are updated frame by
  frame from the frames seen so far (include/danet_online_hip.h), causal in the embedding.  `ONLINE_INIT_FRAMES` (the
  hold length T0 in frames, an integer >= 1, default None = 32 when that estimator is selected: a choice, not a tuned
  value) and `ONLINE_MEMORY_FRAMES` (tau > 0 frames, the forgetting factor being lambda = exp(-1 / tau); default None
  = lambda = 1, the running mean of everything seen) need it; not as `TRAIN_ESTIMATOR_METHOD` (it has no backward) and
  not with `INFER_CHUNK_LEN`.
* `ENCODER_TYPE = "lstm-causal"` selects the causal encoder: the `lstm-orig` stack (same variables, so its parameter
  files load) with both whole-utterance centrings replaced by a running mean over the frames seen so far
  (include/danet_causal_hip.h); the embedding of frame t then depends on frames <= t only.  It trains like `lstm-orig`.
  With it and `INFER_ESTIMATOR_METHOD = "online"`, `Model.open_stream(batch)` returns a session that separates a
  recording block by block as it arrives, and `INFER_STREAM_BLOCK` (an integer in 1..64, default None = off) makes
  `Model.infer` feed the recording through such a session in blocks of that many frames; it needs that encoder and
  that estimator, `BATCH_SIZE` <= 16 when `infer` runs, and not `INFER_CHUNK_LEN` or `PHASE_REFINE_ITERS`;
  `train_step` and `valid_step` never look at it.
* `TRAIN_ESTIMATOR_METHOD = "truth-online"` trains under the conditions `INFER_ESTIMATOR_METHOD = "online"` runs in:
  frame t is separated with the running, forgetting-weighted means of the embedding under the ideal assignment of
  the frames <= t (the first T0 frames share those of frame T0 - 1), with an exact backward
  (include/danet_tonline_hip.h).  It needs `INFER_ESTIMATOR_METHOD = "online"`, whose `ONLINE_INIT_FRAMES` and
  `ONLINE_MEMORY_FRAMES` it shares; no key of its own; not as `INFER_ESTIMATOR_METHOD` (it uses the truth).
* `get_regularizer()` returns None: the reference attaches a regulariser that
  never reaches the loss (`main.py:228-229` vs `:289-290,358`).
'''
import re
import json
import types

import numpy as np
import scipy.signal
import scipy.signal.windows

DEFAULTS = {
    'FLOATX': 'float32',
    'INTX': 'int32',
    'FFT_SIZE': 256,
    'FFT_STRIDE': 64,
    'FFT_WND': 'np.sqrt(scipy.signal.hann(self.FFT_SIZE)).astype(self.FLOATX)',
    'SMPRATE': 8000,
    'BATCH_SIZE': 32,
    'MAX_N_SIGNAL': 2,
    'LENGTH_ALIGN': 4,
    'MAX_TRAIN_LEN': 128,
    'EMBED_SIZE': 20,
    'RELU_LEAKAGE': 0.3,
    'EPS': 1e-7,
    'DROPOUT_KEEP_PROB': 1.0,
    'REG_SCALE': 1e-2,
    'REG_TYPE': 'L2',
    'LR': 3e-4,
    'LR_DECAY': 0.8,
    'LR_DECAY_TYPE': None,
    'NUM_EPOCH_PER_LR_DECAY': 10,
    'GRAD_CLIP_THRES': 100.0,
    'TRAIN_ESTIMATOR_METHOD': 'truth-weighted',
    'INFER_ESTIMATOR_METHOD': 'anchor',
    'NUM_ANCHOR': 6,
    'ENCODER_TYPE': 'toy',
    'SEPARATOR_TYPE': 'dot-sigmoid-orig',
    'OPTIMIZER_TYPE': 'adam',
    'DATASET_TYPE': 'toy',
    'SUMMARY_DIR': './logs',
    'SUMMARY_TITLE': 'Test 1',
    'DEBUG': False,
    # extensions (reference values hard-coded at app/modules.py:212,223-242)
    'NUM_LSTM_LAYERS': 4,
    'LSTM_HDIM': 300,
    # k-means estimator (not in the reference, README.md:216; BASELINE cfg 5)
    'KMEANS_ITERS': 10,
    # root folder of the `wavdir` dataset: DATASET_DIR/{train,valid,test}/**/*.wav (not in the reference)
    'DATASET_DIR': None,
    # mixture level control of the `wavdir` dataset, dB, None = off (not in the reference; include/danet_mix_hip.h)
    'MIX_SNR_RANGE': None,
    'MIX_LEVEL_RANGE': None,
    # speed perturbation of the `wavdir` dataset's train subset, a fraction in [0, 0.25], None = off (not in the
    # reference; include/danet_speed_hip.h)
    'SPEED_PERTURB_RANGE': None,
    # reverberation of the `wavdir` dataset's train subset: the longest RT60 of the bank of room responses, seconds
    # in [0, 1.0], None = off (not in the reference; include/danet_reverb_hip.h)
    'REVERB_RT60_MAX': None,
    # `valid` / `test` also report the SI-SDR of the separated waveforms and its improvement over the mixture, dB:
    # true = on, null / false = off (not in the reference; include/danet_metric_hip.h)
    'EVAL_SI_SDR': None,
    # additive noise in the `wavdir` dataset's train subset: a folder of noise recordings (NOISE_DIR/**/*.wav) and the
    # range the SNR of every mixture is drawn from, dB in [-30, 60]; all three None = off (not in the reference;
    # include/danet_noise_hip.h)
    'NOISE_DIR': None,
    'NOISE_SNR_MIN': None,
    'NOISE_SNR_MAX': None,
    # additive noise in the `wavdir` dataset's valid / test subsets: a folder of held-out noise recordings
    # (NOISE_EVAL_DIR/**/*.wav) and the range the SNR of every mixture is drawn from, dB in [-30, 60]; all three
    # None = off; independent of the three train keys above (not in the reference; include/danet_neval_hip.h)
    'NOISE_EVAL_DIR': None,
    'NOISE_EVAL_SNR_MIN': None,
    'NOISE_EVAL_SNR_MAX': None,
    # what a source's level is in the `wavdir` dataset's MIX_SNR_RANGE / NOISE_SNR_* rules: None = its mean power over
    # the whole file, "active" = its ITU-T P.56 active speech level (not in the reference; include/danet_level_hip.h)
    'MIX_LEVEL_MEASURE': None,
    # what Model.train_step minimises: None / "pit-mse" = the reference's PIT-MSE on complex spectra, "si-sdr" = minus
    # the SI-SDR of the separated waveforms in dB (not in the reference; include/danet_wavloss_hip.h)
    'TRAIN_LOSS': None,
    # the largest global L2 norm of the gradient: beyond it the whole gradient is scaled down to it, ahead of the
    # value clip GRAD_CLIP_THRES; None = off (not in the reference; include/danet_gclip_hip.h)
    'GRAD_CLIP_NORM': None,
    # the weight of the deep-clustering affinity loss of the embedding (magnitude-ratio weights, ideal-binary-mask
    # labels) added to the training loss; None = off, 0.0 = computed and reported but without effect (not in the
    # reference; include/danet_dpcl_hip.h)
    'DPCL_WEIGHT': None,
    # chunked inference of long recordings: the chunk length in frames (a multiple of LENGTH_ALIGN, >= 2), the
    # cross-fade length in frames (1 <= V <= L // 2; None = max(1, L // 4)) and the number of chunks per encoder launch
    # group (>= 1; None = 16); INFER_CHUNK_LEN None = off (not in the reference; include/danet_stitch_hip.h)
    'INFER_CHUNK_LEN': None,
    'INFER_CHUNK_OVERLAP': None,
    'INFER_CHUNK_BATCH': None,
    # `valid` / `test` also report the BSS-eval v3 (bss_eval_sources) SDR, SIR, SAR and the SDR improvement over the
    # mixture, dB: true = on, null / false = off; and the length of the allowed distortion filter, an integer in
    # 1..512, None = 512, which needs the first key (not in the reference; include/danet_bss_hip.h)
    'EVAL_BSS_SDR': None,
    'EVAL_BSS_FILTER_LEN': None,
    # `valid` / `test` also report STOI, ESTOI and the improvement of each over the mixture, on the waveforms
    # resampled to 10 kHz: true = on, null / false = off (not in the reference; include/danet_stoi_hip.h)
    'EVAL_STOI': None,
    # iterations of MISI phase refinement of the separated spectra in `infer` and ahead of the waveform metrics of
    # `valid` / `test`: an integer in 1..100, None = off (not in the reference; include/danet_phase_hip.h)
    'PHASE_REFINE_ITERS': None,
    # the "online" inference estimator (INFER_ESTIMATOR_METHOD = "online"): the hold length T0 in frames, an integer
    # >= 1 (None = 32 when the estimator is selected; a choice, not tuned), and the memory tau > 0 in frames of the
    # forgetting factor lambda = exp(-1 / tau) (None = lambda = 1, the running mean of everything seen); both need that
    # estimator (not in the reference; include/danet_online_hip.h)
    'ONLINE_INIT_FRAMES': None,
    'ONLINE_MEMORY_FRAMES': None,
    # block-wise streaming inference: Model.infer feeds the recording through a Model.open_stream session in blocks of
    # this many frames, an integer in 1..64, None = off; needs ENCODER_TYPE = "lstm-causal" and INFER_ESTIMATOR_METHOD
    # = "online", not with INFER_CHUNK_LEN or PHASE_REFINE_ITERS (not in the reference; include/danet_causal_hip.h)
    'INFER_STREAM_BLOCK': None,
}


class _ScipySignalCompat(types.SimpleNamespace):
    '''scipy.signal with the removed `hann` alias restored for FFT_WND eval.'''
    def __getattr__(self, name):
        if name == 'hann':
            return scipy.signal.windows.hann
        return getattr(scipy.signal, name)


class _ScipyCompat(types.SimpleNamespace):
    signal = _ScipySignalCompat()

    def __getattr__(self, name):
        import scipy as _sp
        return getattr(_sp, name)


class Hyperparameter:
    '''
    Contains hyperparameter settings (reference: app/hparams.py:15-127)
    '''
    pattern = r'[A-Z_][A-Z0-9_]*'      # (digits after the first letter: REVERB_RT60_MAX)

    def __init__(self):
        self.__dict__.update(DEFAULTS)

    def digest(self):
        '''
        Re-derive inferred hyperparams; call after every update
        (reference: app/hparams.py:29-42).
        '''
        self.COMPLEXX = dict(
            float32='complex64', float64='complex128')[self.FLOATX]
        self.FEATURE_SIZE = 1 + self.FFT_SIZE // 2
        assert isinstance(self.DROPOUT_KEEP_PROB, float)
        assert 0. < self.DROPOUT_KEEP_PROB <= 1.
        if isinstance(self.FFT_WND, str):
            self._FFT_WND_EXPR = self.FFT_WND
        expr = getattr(self, '_FFT_WND_EXPR', None)
        if expr is not None:
            self.FFT_WND = eval(
                expr, {'np': np, 'scipy': _ScipyCompat(), 'self': self})

    def load(self, di):
        '''load from a dict (reference: app/hparams.py:44-57)'''
        assert isinstance(di, dict)
        pat = re.compile(self.pattern)
        for k, v in di.items():
            if None is pat.fullmatch(k):
                raise NameError
            assert isinstance(v, (str, int, float, bool, type(None)))
        if 'FFT_WND' in di:
            self.__dict__.pop('_FFT_WND_EXPR', None)
        self.__dict__.update(di)

    def load_json(self, file_):
        '''load from JSON file (reference: app/hparams.py:59-69)'''
        if isinstance(file_, (str, bytes)):
            file_ = open(file_, 'r')
        di = json.load(file_)
        self.load(di)

    def reset(self):
        '''back to default.json values (test helper; not in the reference)'''
        self.__dict__.clear()
        self.__dict__.update(DEFAULTS)

    def get_regularizer(self):
        # reference builds tf.contrib l1/l2 regularisers (app/hparams.py:122-127)
        # whose losses are never added to the training loss; a no-op here.
        return None


# Plugin registries (reference: app/hparams.py:72-120).  One row per plugin
# kind: (kind, registry attribute, hyperparameter that names the active
# plugin or None when the getter takes the name).  The decorators and
# getters the reference spells out one by one are generated from the table.
_PLUGIN_KINDS = (
    ('encoder', 'encoder_registry', 'ENCODER_TYPE'),
    ('estimator', 'estimator_registry', None),
    ('separator', 'separator_registry', None),
    ('optimizer', 'ozer_registry', 'OPTIMIZER_TYPE'),
    ('dataset', 'dataset_registry', 'DATASET_TYPE'),
)


def _install_plugin_kind(kind, attr, selector):
    table = {}
    setattr(Hyperparameter, attr, table)

    def register(cls, name):
        def keep(obj):
            table[name] = obj
            return obj
        return keep
    register.__name__ = 'register_' + kind
    register.__doc__ = 'decorator: add a %s plugin under `name`' % kind
    setattr(Hyperparameter, register.__name__, classmethod(register))

    if selector is None:
        def get(self, name):
            return table[name]
    else:
        def get(self):
            return table[getattr(self, selector)]
    get.__name__ = 'get_' + kind
    setattr(Hyperparameter, get.__name__, get)


for _row in _PLUGIN_KINDS:
    _install_plugin_kind(*_row)


hparams = Hyperparameter()
