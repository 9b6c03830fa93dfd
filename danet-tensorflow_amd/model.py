'''
Model: the forward graph of the reference's `Model.build()` (main.py:208-399)
re-stated eagerly over the HIP ops, plus the train / valid / infer steps the
reference runs through `g_sess.run` (main.py:402-532, :685-690).

Host code is Python + PyTorch-ROCm (autograd engine, device memory, streams,
torch.distributed); every tensor op on the path is a libdanet_hip.so kernel.

Data parallelism (new; the reference is single-GPU, README.md:226): one process
per GPU, `hparams.BATCH_SIZE` is the per-GPU batch, parameters live in one flat
fp32 buffer broadcast from rank 0, gradients accumulate into one flat fp32
bucket that is all-reduced ONCE per step over RCCL, then
value-clipped (main.py:359-362) and applied by the TF1-style Adam kernel.
'''
import math
import os

import numpy as np
import torch

from .hparams import hparams
from . import _lib, ops
from . import modules  # noqa: F401  (registers the plugins)
from . import ozers    # noqa: F401  (registers the optimisers)
from . import dist


class Model(object):
    '''Base class for a fully trainable model (main.py:61-548)'''

    def __init__(self, name='BaseModel', device=None, seed=1337, grad_schedule=None):
        '''grad_schedule (data parallelism only; default: env DANET_OVERLAP_ALLREDUCE or 'auto'):
        '0' = ONE all-reduce of the flat gradient bucket after backward (the north_star
        form); 'tail' = two collectives (everything outside the bottom encoder layer under
        that layer's weight-gradient GEMMs, the rest after backward); '1' = per-layer buckets
        under the remaining BPTT kernels (opt-in only).  'auto' (default) starts as '0' and
        DECIDES between '0' and 'tail' after AUTO_DECIDE_AT train steps from two measurements of
        its own -- the stand-alone all-reduce time of its bucket and its step time, MAX-reduced
        over the ranks -- with one threshold (dist.choose_schedule, DANET_ALLREDUCE_TAIL_RATIO);
        `schedule_decision` records what was measured.  Without a process group 'auto' is '0'.'''
        self.grad_schedule = str(grad_schedule if grad_schedule is not None else
                                 os.environ.get('DANET_OVERLAP_ALLREDUCE', 'auto'))
        assert self.grad_schedule in ('0', 'tail', '1', 'auto'), self.grad_schedule
        self.schedule_decision = None
        self._auto = self.grad_schedule == 'auto'
        if self._auto:
            self.grad_schedule = '0'
        self.name = name
        self.device = torch.device(device if device is not None else
                                   'cuda:%d' % torch.cuda.current_device())
        self.s_states_di = {}
        self.vars = {}
        self._order = []
        self.seed = int(seed)
        self._gen = torch.Generator().manual_seed(seed)
        self._dropout = None
        self._noise = None          # (s_noise, s_noise_gain) while forward_noisy() builds its forward pass
        self._flat = None
        self.learn_rate = float(hparams.LR)
        self.step_count = 0
        # train steps taken before the parameter file this model was loaded from was written: the
        # dropout masks' `step` word is step_base + step_count, so a resumed run continues the mask
        # sequence, while Adam's own step (step_count) restarts with its moments, which are not in
        # the file (trainables only, like the reference's Saver)
        self.step_base = 0
        self.built = False
        # True: gradients stay readable after train_step (grad_dict); costs one fill
        # kernel per step.  False: the optimiser kernel zeroes them after use.
        self.keep_grads = False
        # train_step: separator + PIT loss as one fused kernel pair (DANET_FUSE_HEADS=0: off)
        self.fuse_heads = os.environ.get('DANET_FUSE_HEADS', '1') == '1'
        # what train_step minimises: build() sets it from hparams.TRAIN_LOSS ('pit-mse' or 'si-sdr')
        self.train_loss = 'pit-mse'
        self.grad_clip_norm = None
        self._gclip_partials = None
        # None: off; a float: the weight of the deep-clustering auxiliary loss (build() sets it from DPCL_WEIGHT)
        self.dpcl_weight = None
        # None: off; (L, V, G): chunk length, cross-fade and chunks per launch group of chunked inference (build() sets
        # it from INFER_CHUNK_LEN / INFER_CHUNK_OVERLAP / INFER_CHUNK_BATCH)
        self.infer_chunk = None
        # None: off; an int: the iterations of MISI phase refinement (build() sets it from PHASE_REFINE_ITERS)
        self.phase_refine = None
        # None: the inference estimator is not "online"; (T0, lambda): its hold length in frames and its forgetting
        # factor (build() sets it from ONLINE_INIT_FRAMES / ONLINE_MEMORY_FRAMES)
        self.online = None
        # None: off; an int: the frames per block Model.infer feeds through a stream session (build() sets it from
        # INFER_STREAM_BLOCK)
        self.stream_block = None

    # ------------------------------------------------------------ variables
    def get_variable(self, name, shape, init):
        '''tf.get_variable under scope "global/" (main.py:229).  `init(shape,
        generator)` returns a CPU float32 tensor.'''
        full = 'global/' + name
        v = self.vars.get(full)
        if v is None:
            if self._flat is not None:
                raise KeyError('variable %s requested after build()' % full)
            v = init(list(shape), self._gen).to(self.device).requires_grad_(True)
            assert list(v.shape) == list(shape), (full, v.shape, shape)
            self.vars[full] = v
            self._order.append(full)
        return v

    def lyr_lstm(self, name, s_x, hdim, axis=-1, t_axis=0, op_linear=None,
                 w_init=None, b_init=None):
        '''single unidirectional LSTM layer (main.py:76-132); s_x [B,T,D]
        (t_axis=-2/1) or [T,B,D] (t_axis=0) -> same layout with D -> hdim.
        Zero initial state; state variables are never carried across calls
        (main.py:108-123, :538-540).'''
        assert s_x.dim() == 3 and axis in (-1, 2)
        t_axis = t_axis % 3
        assert t_axis in (0, 1)
        if t_axis == 0:
            s_x = s_x.transpose(0, 1)
        D = s_x.shape[-1]
        W = self.get_variable(name + '/LSTM/linear/W', [D + hdim, 4 * hdim], w_init)
        b = self.get_variable(name + '/LSTM/linear/B', [4 * hdim], b_init)
        y = ops.LstmLayerFn.apply(s_x, hdim, W, b)
        return y.transpose(0, 1) if t_axis == 0 else y

    def parameter_count(self):
        return sum(v.numel() for v in self.vars.values())

    # ---------------------------------------------------------------- build
    def build(self):
        '''create sub-modules (main.py:210-211, 249-250, 263-270), materialise
        variables with one dry forward, then flatten them for the optimiser.'''
        self.eval_si_sdr = self._check_eval_si_sdr()
        # None: off; an int: the filter length L of the BSS-eval figures (include/danet_bss_hip.h)
        self.eval_bss = self._check_eval_bss()
        # STOI / ESTOI of the separated waveforms (include/danet_stoi_hip.h)
        self.eval_stoi = self._check_eval_stoi()
        # None: off; an int: the iterations of MISI phase refinement (include/danet_phase_hip.h)
        self.phase_refine = self._check_phase_refine()
        # 'pit-mse': the reference's PIT-MSE on complex spectra; 'si-sdr': -SI-SDR of the separated waveforms
        self.train_loss = self._check_train_loss()
        # None: off; a float: the largest global L2 norm of the gradient (include/danet_gclip_hip.h)
        self.grad_clip_norm = self._check_grad_clip_norm()
        self._gclip_partials = None
        # None: off; a float >= 0: the weight of the deep-clustering auxiliary loss (include/danet_dpcl_hip.h)
        self.dpcl_weight = self._check_dpcl_weight()
        # None: off; (L, V, G) of chunked inference (include/danet_stitch_hip.h)
        self.infer_chunk = self._check_infer_chunk()
        # None: off; (T0, lambda) of the "online" inference estimator (include/danet_online_hip.h)
        self.online = self._check_online()
        # None: off; an int in 1..64: infer goes through a stream session in blocks of that many frames
        # (include/danet_causal_hip.h)
        self.stream_block = self._check_stream_block()
        self.encoder = hparams.get_encoder()(self, 'encoder')
        self.estimator = hparams.get_estimator(
            hparams.TRAIN_ESTIMATOR_METHOD)(self, 'train_estimator')
        self.using_same_method = (
            hparams.INFER_ESTIMATOR_METHOD == hparams.TRAIN_ESTIMATOR_METHOD)
        if self.using_same_method:
            self.valid_estimator = self.estimator
        else:
            self.valid_estimator = hparams.get_estimator(
                hparams.INFER_ESTIMATOR_METHOD)(self, 'infer_estimator')
            assert not self.valid_estimator.USE_TRUTH           # main.py:266
        self.separator = hparams.get_separator(hparams.SEPARATOR_TYPE)(self, 'separator')
        B, C, F = hparams.BATCH_SIZE, hparams.MAX_N_SIGNAL, hparams.FEATURE_SIZE
        dry = torch.zeros(B, C, 4, F, dtype=torch.complex64, device=self.device)
        with torch.no_grad():
            self.forward(dry, with_valid=True)
        self._flatten()
        self.ozer = hparams.get_optimizer()(
            learn_rate=self.learn_rate, lr_decay=hparams.LR_DECAY)
        self.ozer.bind(self._flat, self._flat_grad)
        self.built = True
        dist.broadcast_params_(self._flat)
        ops.weights_written(self._flat)
        return self

    @staticmethod
    def _check_eval_si_sdr():
        '''EVAL_SI_SDR (null / false: off) -> bool; ValueError naming the key that rules the metric out'''
        v = getattr(hparams, 'EVAL_SI_SDR', None)
        if v is not None and not isinstance(v, bool):
            raise ValueError('EVAL_SI_SDR must be null, true or false (got %r)' % (v,))
        if not v:
            return False
        Model._check_synth_envelope('EVAL_SI_SDR', ops.METRIC_MAX_C)
        return True

    @staticmethod
    def _check_synth_envelope(key, max_c):
        '''the envelope of danet_metric_synth, whose waveforms the metric `key` is taken on; ValueError naming `key`'''
        N, S = hparams.FFT_SIZE, hparams.FFT_STRIDE
        if N < 64 or N > 1024 or N & (N - 1):
            raise ValueError('%s needs FFT_SIZE to be a power of two in 64..1024 (got FFT_SIZE = %d): the '
                             'envelope of danet_metric_synth' % (key, N))
        if 2 * S > N:
            raise ValueError('%s needs FFT_STRIDE <= FFT_SIZE / 2 (got FFT_STRIDE = %d at FFT_SIZE = %d): '
                             'beyond half a window the overlap-added squared window can reach 0 at the window '
                             'edges' % (key, S, N))
        if 8 * S < N:
            raise ValueError('%s needs FFT_STRIDE >= FFT_SIZE / 8 (got FFT_STRIDE = %d at FFT_SIZE = %d): '
                             'the frames that overlap one tile of hops must fit in the 64 KiB of LDS the synthesis '
                             'kernel uses' % (key, S, N))
        if hparams.MAX_N_SIGNAL > max_c:
            raise ValueError('%s needs MAX_N_SIGNAL <= %d (got %d)' % (key, max_c, hparams.MAX_N_SIGNAL))

    @staticmethod
    def _check_eval_bss():
        '''EVAL_BSS_SDR / EVAL_BSS_FILTER_LEN (null / false: off) -> None or the filter length L; ValueError naming the
        key that rules the metric out'''
        v = getattr(hparams, 'EVAL_BSS_SDR', None)
        if v is not None and not isinstance(v, bool):
            raise ValueError('EVAL_BSS_SDR must be null, true or false (got %r)' % (v,))
        L = getattr(hparams, 'EVAL_BSS_FILTER_LEN', None)
        if L is not None and (isinstance(L, bool) or not isinstance(L, int) or L < 1 or L > ops.BSS_MAX_L):
            raise ValueError('EVAL_BSS_FILTER_LEN must be null or an integer in 1..%d (got %r)' % (ops.BSS_MAX_L, L))
        if not v:
            if L is not None:
                raise ValueError('EVAL_BSS_FILTER_LEN is set but EVAL_BSS_SDR is not: the filter length needs the metric')
            return None
        if getattr(hparams, 'NOISE_EVAL_DIR', None) is not None:
            raise ValueError('EVAL_BSS_SDR cannot be combined with NOISE_EVAL_DIR: the BSS-eval baseline of a noisy '
                             'mixture is not implemented')
        # the waveforms are those of danet_metric_synth: EVAL_SI_SDR's rules, under this key's name
        Model._check_synth_envelope('EVAL_BSS_SDR', min(ops.BSS_MAX_C, ops.METRIC_MAX_C))
        return ops.BSS_MAX_L if L is None else L

    @staticmethod
    def _check_eval_stoi():
        '''EVAL_STOI (null / false: off) -> bool; ValueError naming the key that rules the metric out'''
        v = getattr(hparams, 'EVAL_STOI', None)
        if v is not None and not isinstance(v, bool):
            raise ValueError('EVAL_STOI must be null, true or false (got %r)' % (v,))
        if not v:
            return False
        if getattr(hparams, 'NOISE_EVAL_DIR', None) is not None:
            raise ValueError('EVAL_STOI cannot be combined with NOISE_EVAL_DIR: the intelligibility baseline of a '
                             'noisy mixture is not implemented')
        # the waveforms are those of danet_metric_synth: EVAL_SI_SDR's rules, under this key's name
        Model._check_synth_envelope('EVAL_STOI', min(ops.STOI_MAX_C, ops.METRIC_MAX_C))
        ops.stoi_rate(hparams.SMPRATE)                       # ValueError naming EVAL_STOI and SMPRATE
        return True

    _stoi_key = _check_eval_stoi

    @staticmethod
    def _check_phase_refine():
        '''PHASE_REFINE_ITERS (null: off) -> None or the iteration count; ValueError naming the key that rules it out'''
        v = getattr(hparams, 'PHASE_REFINE_ITERS', None)
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, int) or v < 1 or v > 100:
            raise ValueError('PHASE_REFINE_ITERS must be null or an integer in 1..100 (got %r)' % (v,))
        if getattr(hparams, 'NOISE_EVAL_DIR', None) is not None:
            raise ValueError('PHASE_REFINE_ITERS cannot be combined with NOISE_EVAL_DIR: the refined sources sum to the '
                             'mixture, so the noise of a noisy mixture would be shared among them')
        # the waveforms are those of danet_metric_synth: EVAL_SI_SDR's rules, under this key's name
        Model._check_synth_envelope('PHASE_REFINE_ITERS', ops.PHASE_MAX_C)
        return v

    @staticmethod
    def _check_train_loss():
        '''TRAIN_LOSS (null = "pit-mse") -> 'pit-mse' or 'si-sdr'; ValueError naming the key that rules the choice out'''
        v = getattr(hparams, 'TRAIN_LOSS', None)
        if v is None:
            return 'pit-mse'
        if not isinstance(v, str) or v not in ('pit-mse', 'si-sdr'):
            raise ValueError('TRAIN_LOSS must be null, "pit-mse" or "si-sdr" (got %r)' % (v,))
        if v == 'pit-mse':
            return v
        N, S = hparams.FFT_SIZE, hparams.FFT_STRIDE
        if N < 64 or N > 1024 or N & (N - 1):
            raise ValueError('TRAIN_LOSS = "si-sdr" needs FFT_SIZE to be a power of two in 64..1024 (got FFT_SIZE = %d): '
                             'the envelope of danet_metric_synth, whose waveforms the loss is taken on' % N)
        if 2 * S > N:
            raise ValueError('TRAIN_LOSS = "si-sdr" needs FFT_STRIDE <= FFT_SIZE / 2 (got FFT_STRIDE = %d at FFT_SIZE '
                             '= %d): beyond half a window the overlap-added squared window can reach 0 at the window '
                             'edges' % (S, N))
        if 8 * S < N:
            raise ValueError('TRAIN_LOSS = "si-sdr" needs FFT_STRIDE >= FFT_SIZE / 8 (got FFT_STRIDE = %d at FFT_SIZE '
                             '= %d): the frames that overlap one tile of hops must fit in the 64 KiB of LDS the '
                             'synthesis kernel uses' % (S, N))
        if hparams.MAX_N_SIGNAL > ops.WAVLOSS_MAX_C:
            raise ValueError('TRAIN_LOSS = "si-sdr" needs MAX_N_SIGNAL <= %d (got %d)'
                             % (ops.WAVLOSS_MAX_C, hparams.MAX_N_SIGNAL))
        return v

    @staticmethod
    def _check_grad_clip_norm():
        '''GRAD_CLIP_NORM (null: off) -> None or a float; ValueError naming the key'''
        v = getattr(hparams, 'GRAD_CLIP_NORM', None)
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError('GRAD_CLIP_NORM must be null or a number > 0 (got %r)' % (v,))
        if not math.isfinite(v) or v <= 0:
            raise ValueError('GRAD_CLIP_NORM must be null or a finite number > 0 (got %r)' % (v,))
        if _lib.expert('early_adam', False):
            raise ValueError('GRAD_CLIP_NORM cannot be combined with the expert setting early_adam: the early optimizer '
                             'piece would run before the norm of the whole gradient exists')
        return float(v)

    @staticmethod
    def _check_dpcl_weight():
        '''DPCL_WEIGHT (null: off) -> None or a float >= 0; ValueError naming the key that rules the value out'''
        v = getattr(hparams, 'DPCL_WEIGHT', None)
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError('DPCL_WEIGHT must be null or a number >= 0 (got %r)' % (v,))
        if not math.isfinite(v) or v < 0:
            raise ValueError('DPCL_WEIGHT must be null or a finite number >= 0 (got %r)' % (v,))
        if hparams.EMBED_SIZE > ops.DPCL_MAX_E:
            raise ValueError('DPCL_WEIGHT needs EMBED_SIZE <= %d (got %d)' % (ops.DPCL_MAX_E, hparams.EMBED_SIZE))
        if hparams.MAX_N_SIGNAL > ops.DPCL_MAX_C:
            raise ValueError('DPCL_WEIGHT needs MAX_N_SIGNAL <= %d (got %d)' % (ops.DPCL_MAX_C, hparams.MAX_N_SIGNAL))
        return float(v)

    @staticmethod
    def _check_infer_chunk():
        '''INFER_CHUNK_LEN / INFER_CHUNK_OVERLAP / INFER_CHUNK_BATCH (all null: off) -> None or (L, V, G); ValueError
        naming the key that rules the values out'''
        def integer(key, least):
            v = getattr(hparams, key, None)
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < least):
                raise ValueError('%s must be null or an integer >= %d (got %r)' % (key, least, v))
            return v
        L = integer('INFER_CHUNK_LEN', 2)
        V = integer('INFER_CHUNK_OVERLAP', 1)
        G = integer('INFER_CHUNK_BATCH', 1)
        if L is None:
            for key, v in (('INFER_CHUNK_OVERLAP', V), ('INFER_CHUNK_BATCH', G)):
                if v is not None:
                    raise ValueError('%s is set (%r) while INFER_CHUNK_LEN is null: it needs INFER_CHUNK_LEN' % (key, v))
            return None
        if L % hparams.LENGTH_ALIGN:
            raise ValueError('INFER_CHUNK_LEN must be a multiple of LENGTH_ALIGN = %d (got %d)'
                             % (hparams.LENGTH_ALIGN, L))
        if V is None:
            V = max(1, L // 4)
        if V > L // 2:
            raise ValueError('INFER_CHUNK_OVERLAP must be in 1 .. INFER_CHUNK_LEN // 2 = %d (got %d)' % (L // 2, V))
        if hparams.MAX_N_SIGNAL > ops.STITCH_MAX_C:
            raise ValueError('INFER_CHUNK_LEN needs MAX_N_SIGNAL <= %d (got %d): the stitching searches at most 24 '
                             'permutations per pair of chunks' % (ops.STITCH_MAX_C, hparams.MAX_N_SIGNAL))
        return L, V, 16 if G is None else G

    @staticmethod
    def _check_online():
        '''INFER_ESTIMATOR_METHOD = "online" with ONLINE_INIT_FRAMES / ONLINE_MEMORY_FRAMES -> None (another estimator)
        or (T0, lambda), lambda = exp(-1 / ONLINE_MEMORY_FRAMES) formed in float64; ValueError naming the keys that rule
        the choice out'''
        t0 = getattr(hparams, 'ONLINE_INIT_FRAMES', None)
        tau = getattr(hparams, 'ONLINE_MEMORY_FRAMES', None)
        if t0 is not None and (isinstance(t0, bool) or not isinstance(t0, int) or t0 < 1):
            raise ValueError('ONLINE_INIT_FRAMES must be null or an integer >= 1 (got %r)' % (t0,))
        if tau is not None and (isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau)
                                or tau <= 0):
            raise ValueError('ONLINE_MEMORY_FRAMES must be null or a finite number > 0 (got %r)' % (tau,))
        if hparams.TRAIN_ESTIMATOR_METHOD == 'online':
            raise ValueError('TRAIN_ESTIMATOR_METHOD cannot be "online": the online estimator has no backward, it is an '
                             'inference estimator (INFER_ESTIMATOR_METHOD)')
        if hparams.TRAIN_ESTIMATOR_METHOD == 'truth-online' and hparams.INFER_ESTIMATOR_METHOD != 'online':
            raise ValueError('TRAIN_ESTIMATOR_METHOD = "truth-online" needs INFER_ESTIMATOR_METHOD = "online" (got %r): it '
                             'is the training twin of that estimator and takes its hold length and forgetting factor '
                             '(ONLINE_INIT_FRAMES / ONLINE_MEMORY_FRAMES) from it' % (hparams.INFER_ESTIMATOR_METHOD,))
        if hparams.INFER_ESTIMATOR_METHOD != 'online':
            for key, v in (('ONLINE_INIT_FRAMES', t0), ('ONLINE_MEMORY_FRAMES', tau)):
                if v is not None:
                    raise ValueError('%s is set (%r) while INFER_ESTIMATOR_METHOD is %r: it needs INFER_ESTIMATOR_METHOD '
                                     '= "online"' % (key, v, hparams.INFER_ESTIMATOR_METHOD))
            return None
        if getattr(hparams.get_separator(hparams.SEPARATOR_TYPE), 'ACT', None) is None:
            raise ValueError('INFER_ESTIMATOR_METHOD = "online" needs a separator that exposes its activation (ACT, the '
                             'dot-product separators); SEPARATOR_TYPE = %r does not' % (hparams.SEPARATOR_TYPE,))
        if getattr(hparams, 'INFER_CHUNK_LEN', None) is not None:
            raise ValueError('INFER_ESTIMATOR_METHOD = "online" cannot be combined with INFER_CHUNK_LEN: every chunk '
                             'would restart the track')
        for key, v, most in (('MAX_N_SIGNAL', hparams.MAX_N_SIGNAL, ops.ONLINE_MAX_C),
                             ('EMBED_SIZE', hparams.EMBED_SIZE, ops.ONLINE_MAX_E),
                             ('FFT_SIZE', hparams.FFT_SIZE, 2 * (ops.ONLINE_MAX_F - 1))):
            if v > most:
                raise ValueError('INFER_ESTIMATOR_METHOD = "online" needs %s <= %d (got %d)' % (key, most, v))
        lam = 1.0 if tau is None else math.exp(-1.0 / float(tau))
        if not lam > 0.0:
            raise ValueError('ONLINE_MEMORY_FRAMES = %r is too small: exp(-1 / tau) underflows to 0' % (tau,))
        return (32 if t0 is None else t0), lam

    @staticmethod
    def _check_stream_block():
        '''INFER_STREAM_BLOCK (null: off) -> None or the frames per block; ValueError naming the keys that rule it out'''
        v = getattr(hparams, 'INFER_STREAM_BLOCK', None)
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= ops.CAUSAL_MAX_TB:
            raise ValueError('INFER_STREAM_BLOCK must be null or an integer in 1..%d (got %r)' % (ops.CAUSAL_MAX_TB, v))
        Model._check_stream_model('INFER_STREAM_BLOCK')
        for key in ('INFER_CHUNK_LEN', 'PHASE_REFINE_ITERS'):
            if getattr(hparams, key, None) is not None:
                raise ValueError('INFER_STREAM_BLOCK cannot be combined with %s: a stream session decides every frame '
                                 'when it arrives, and both of them need the whole recording' % key)
        return v

    @staticmethod
    def _check_stream_model(who):
        '''what a stream session needs of the configuration; ValueError naming `who` and the key in its way'''
        if hparams.ENCODER_TYPE != 'lstm-causal':
            raise ValueError('%s needs ENCODER_TYPE = "lstm-causal" (got %r): the other encoders see the whole '
                             'recording' % (who, hparams.ENCODER_TYPE))
        if hparams.INFER_ESTIMATOR_METHOD != 'online':
            raise ValueError('%s needs INFER_ESTIMATOR_METHOD = "online" (got %r): the other estimators form one '
                             'attractor set from the whole recording' % (who, hparams.INFER_ESTIMATOR_METHOD))
        if getattr(hparams.get_separator(hparams.SEPARATOR_TYPE), 'ACT', None) is None:
            raise ValueError('%s needs a separator that exposes its activation (ACT, the dot-product separators); '
                             'SEPARATOR_TYPE = %r does not' % (who, hparams.SEPARATOR_TYPE))

    def open_stream(self, batch=1):
        '''a SeparationStream over `batch` recordings that arrive block by block (ENCODER_TYPE = "lstm-causal",
        INFER_ESTIMATOR_METHOD = "online", a dot-product separator, batch <= 16; anything else is a ValueError that names
        the key)'''
        return SeparationStream(self, batch)

    def _separate(self, s_mix_pwr, s_attractors, s_embed_flat):
        '''the separated magnitudes [B, C, T, F] of the validation branch and of infer: a trajectory of attractors
        [B, T, C, E] (the "online" estimator past its hold) goes to ops.online_separate, one attractor set [B, C, E] to
        the separator as ever'''
        if s_attractors.dim() == 4:
            return ops.online_separate(s_mix_pwr, s_attractors, s_embed_flat, self.separator.ACT)
        return self.separator(s_mix_pwr, s_attractors, s_embed_flat)

    def _flatten(self):
        n = sum(self.vars[k].numel() for k in self._order)
        flat = torch.empty(n, device=self.device)
        # 4 spare floats IN FRONT of the gradients: under data parallelism they carry the
        # persistent kernels' hand-off status through the gradient all-reduce (ops.py).  In front,
        # because the variables are laid out bottom encoder layer first: the LAST collective of
        # every schedule ('0': the whole bucket; 'tail': the bottom layer's range, reduced after
        # backward) then covers them as part of one contiguous range -- behind every kernel of the
        # step, wherever a schedule launches its early pieces (round 6; behind the gradients they
        # travelled with 'tail''s early piece, safe only as long as that piece starts after the
        # last recurrent kernel)
        self._grad_store = torch.zeros(n + 4, device=self.device)
        grad = self._grad_store[4:]
        off = 0
        for k in self._order:
            v = self.vars[k]
            m = v.numel()
            flat[off:off + m].copy_(v.detach().reshape(-1))
            nv = flat[off:off + m].view(v.shape).requires_grad_(True)
            nv.grad = grad[off:off + m].view(v.shape)
            self.vars[k] = nv
            off += m
        self._flat, self._flat_grad = flat, grad
        ops.drop_packs(self.device)       # (the dry run packed weights at their old addresses)
        self._one = torch.ones((), device=self.device)
        # a backward pass outside train_step (tests, user code) leaves gradients behind:
        # autograd's accumulation marks the bucket dirty so the next train_step clears it
        self._grads_clean = True
        import weakref
        me = weakref.ref(self)

        def _mark_dirty(_p):
            m = me()
            if m is not None:
                m._grads_clean = False
        for k in self._order:
            self.vars[k].register_post_accumulate_grad_hook(_mark_dirty)
        # gradient reduction schedule (dist.py, see __init__): '0' = one all-reduce after backward;
        # 'tail' / '1' = overlapped pieces; 'auto' starts as '0' and decides after a few steps
        self._buckets = None
        offs, off = {}, 0
        for k in self._order:
            v = self.vars[k]
            offs[v.data_ptr()] = (off, off + v.numel())
            off += v.numel()
        self._offs = offs
        self._install_schedule(self.grad_schedule)
        if self._auto and not dist.is_dist():
            self._auto = False            # nothing to decide without a process group
            self.schedule_decision = dict(schedule='0', reason='single process')
        self._auto_ev = None
        # early optimizer step (opt-in: DANET_EXPERT early_adam=1): once the bottom encoder layer's BPTT
        # kernel has been issued every other gradient is final (and, under data parallelism with
        # the 'tail' schedule, reduced), so clip + Adam over everything outside that layer's range
        # can run on the side stream under the bottom layer's kernels; after backward only the
        # bottom layer's range is left.  The update is elementwise and nothing reads those
        # parameters again in this step (bit-identical parameters, tested).  Round 2 measured
        # -35 us per cfg-2 step; with round 3's shorter tail it LOSES 27 us (3.166 vs 3.192 ms:
        # the 188 MB Adam stream beside the bottom layer's weight-gradient group costs the group
        # more than the 33 us the single update takes afterwards) -> off by default.
        self._early_hooked = False
        self._early_adam = _lib.expert('early_adam', False)
        if dist.is_dist():
            # the status word rides in the gradient all-reduce: every rank sees the same value
            ops.set_status_word(self.device, self._grad_store[:4].view(torch.int32))
        elif ops.status_word(self.device).is_cuda and ops.STATUS_HOST:
            ops.set_status_word(self.device, None)     # a previous data-parallel model's word
        self._early = None          # (ranges, stream) of this step's early update
        self.early_steps = 0        # steps that took the early path (diagnostics / tests)
        self._in_step = False

    # ---- 'auto': '0' or 'tail', decided from the model's own measurements ------------------------
    AUTO_DECIDE_AT = 6       # train steps before the decision; steps 4..6 are the timed ones

    def _install_schedule(self, mode):
        self.grad_schedule = mode
        if mode in ('1', 'tail') and self._buckets is None:
            cls = dist.GradBuckets if mode == '1' else dist.TailOverlap
            if dist.is_dist():      # ranges inside the store: 4 status words in front, reduced LAST
                offs = {k: (lo + 4, hi + 4) for k, (lo, hi) in self._offs.items()}
                self._buckets = cls(self._grad_store, offs, last=[(0, 4)])
            else:
                self._buckets = cls(self._flat_grad, self._offs)
            ops.add_grad_ready_hook(self._buckets.hook)

    def _auto_tick(self):
        '''called at the end of every train step while the schedule is undecided.  Every rank runs
        the same steps, so every rank reaches the decision -- which contains collectives -- at the
        same point; the inputs are MAX-reduced, so every rank decides the same.'''
        n = self.step_count
        if n == self.AUTO_DECIDE_AT - 3:
            self._auto_ev = torch.cuda.Event(enable_timing=True)
            self._auto_ev.record()
        if n < self.AUTO_DECIDE_AT or self._auto_ev is None:
            return
        end = torch.cuda.Event(enable_timing=True)
        end.record()
        end.synchronize()
        step_ms = dist.allreduce_max_scalar(self._auto_ev.elapsed_time(end) / 3.0, self.device)
        ar_ms = dist.measure_allreduce_ms(self._grad_store.numel(), self.device)
        mode = dist.choose_schedule(ar_ms, step_ms)
        self.schedule_decision = dict(schedule=mode, allreduce_ms=round(ar_ms, 4), step_ms=round(step_ms, 4),
                                      ratio=round(ar_ms / step_ms, 5), threshold=dist.TAIL_RATIO,
                                      bucket_bytes=4 * self._grad_store.numel(), decided_at_step=n,
                                      world=dist.world_size())
        self._auto, self._auto_ev = False, None
        self._install_schedule(mode)

    # (the gradient-ready hook is registered only when the early step is wanted: with no hook at
    # all ops does not fire the 'rest' event, whose cross-stream wait costs the main stream ~10 us)
    @property
    def _early_adam(self):
        return self._early_adam_on

    @_early_adam.setter
    def _early_adam(self, on):
        self._early_adam_on = bool(on)
        if on and not self._early_hooked:
            ops.add_grad_ready_hook(self._grad_ready)     # after the bucket's hook: it launches first
            self._early_hooked = True

    def _grad_ready(self, tag, params):
        if self.grad_clip_norm is not None:
            return                      # the norm of the whole gradient does not exist yet
        if tag[0] != 'rest' or not self._early_adam or not self._in_step or self._early is not None:
            return
        rng = [self._offs.get(p.data_ptr()) for p in params]
        if any(r is None for r in rng):
            return                      # not this model's encoder
        if dist.is_dist():
            if not isinstance(self._buckets, dist.TailOverlap):
                return                  # the other schedules reduce these gradients later
            self._buckets.wait_launched()
        ranges = dist._complement(rng, self._flat_grad.numel())
        self.ozer.step(self.step_count + 1, self.learn_rate, clip=hparams.GRAD_CLIP_THRES,
                       grad_scale=1.0 / dist.world_size(), zero_grad=not self.keep_grads,
                       ranges=ranges)
        ops.repack_weights(self.device)
        self._early = (ranges, torch.cuda.current_stream(self.device))
        self.early_steps += 1

    # -------------------------------------------------------------- forward
    def dropout_spec(self, keep):
        '''the ops.DropoutSpec of the step being built: Philox key (seed & 0xffffffff, data-parallel
        rank), step = step_base + step_count at the start of the step.  One spec per forward pass
        (Model.forward resets it), shared by every dropout site so their stream ids differ.'''
        if self._dropout is None or self._dropout.keep != float(keep):
            self._dropout = ops.DropoutSpec(keep, self.seed & 0xffffffff, dist.rank(),
                                            self.step_base + self.step_count)
        return self._dropout

    def forward(self, s_src_signals, with_valid=False, with_train=True, fuse_heads=False,
                s_dropout_keep=1.0):
        '''main.py:215-337.  s_src_signals complex64 [B, C, T, F].
        s_dropout_keep: the keep probability the encoder is called with (the reference feeds
        hparams.DROPOUT_KEEP_PROB on train steps and 1.0 otherwise, main.py:429,490,520, but
        drops it at main.py:243; here it reaches the encoder).  1.0: no dropout, today's path.
        fuse_heads (train_step): separator + phase re-attach + PIT loss + SNR run as ONE
        kernel forward and ONE backward (ops.SeparatePitFn); the separated magnitudes then
        exist only in registers and `sep_pwr` is not in the returned dict.  Needs a separator
        that exposes its activation (`ACT`, the dot-product separators); others take the
        unfused path.  A model built with TRAIN_LOSS = "si-sdr" (`train_loss`) always takes the unfused heads and
        returns the waveform loss as `loss`, with its own permutation in `loss_perm_idx`.  A model built with
        DPCL_WEIGHT set (`dpcl_weight`) returns main loss + weight * deep-clustering loss as `loss` on every head
        path, and the deep-clustering loss alone as `dpcl`.  A model built with TRAIN_ESTIMATOR_METHOD = "truth-online"
        gets a trajectory of attractors [B, T, C, E] from its estimator: it takes the unfused heads whatever fuse_heads
        says, and `attrs` is the trajectory.'''
        B, E = hparams.BATCH_SIZE, hparams.EMBED_SIZE
        eps = float(hparams.EPS)
        if self._noise is None:
            fe = ops.frontend(s_src_signals)                   # main.py:233-240
        else:                                                  # (forward_noisy)
            fe = ops.noise_frontend(s_src_signals, *self._noise)
        self._dropout = None
        if s_dropout_keep < 1.0:
            s_embed = self.encoder(fe['mix_log'], s_dropout_keep)
        else:
            s_embed = self.encoder(fe['mix_log'])              # main.py:243
        s_embed_flat = s_embed.reshape(B, -1, E)               # main.py:244-246
        out = dict(embed=s_embed, input=s_src_signals)
        phasor = fe['phasor']
        if with_train:
            s_attractors = self.estimator(                     # main.py:251-254
                s_embed, s_src_pwr=fe['src_pwr'], s_mix_pwr=fe['mix_pwr'])
            act = getattr(self.separator, 'ACT', None)
            # "truth-online" returns per-frame attractors [B, T, C, E]: the unfused heads with ops.OnlineSeparateFn in
            # the separator's place (the fused heads take one attractor set)
            traj = s_attractors.dim() == 4
            if self.dpcl_weight is not None:
                ops.unshare_dembed(s_attractors)       # the embedding gets a third consumer below
            if self.train_loss == 'si-sdr':
                # the waveform loss needs the separated magnitudes: the unfused heads.  SNR, perm_idx and perms keep
                # their meaning (one more launch, outside autograd); the loss's own permutation is loss_perm_idx
                s_sep_pwr = (ops.OnlineSeparateFn.apply(fe['mix_pwr'], s_attractors, s_embed_flat, act) if traj else
                             self.separator(fe['mix_pwr'], s_attractors, s_embed_flat))
                loss, loss_idx = ops.si_sdr_loss(s_src_signals, s_sep_pwr, phasor)
                with torch.no_grad():
                    _mse, perms, idx, snr = ops.pit_mse_loss(
                        s_src_signals, s_sep_pwr.detach(), phasor, mode=0, eps=eps)
                out.update(attrs=s_attractors, sep_pwr=s_sep_pwr, loss=loss, SNR=snr,
                           perm_idx=idx, perms=perms, loss_perm_idx=loss_idx)
            elif fuse_heads and act is not None and not hparams.DEBUG and not with_valid and not traj:
                loss, perms, idx, snr = ops.separate_pit_loss(      # :271-272 + :281-290, 308-309
                    fe['mix_pwr'], s_attractors, s_embed_flat, s_src_signals, phasor, act,
                    mode=0, eps=eps)
                out.update(attrs=s_attractors, loss=loss, SNR=snr, perm_idx=idx, perms=perms)
            else:
                s_sep_pwr = (ops.OnlineSeparateFn.apply(fe['mix_pwr'], s_attractors, s_embed_flat, act) if traj else
                             self.separator(fe['mix_pwr'], s_attractors, s_embed_flat))  # :271-272
                loss, perms, idx, snr = ops.pit_mse_loss(          # main.py:289-290, 308-309
                    s_src_signals, s_sep_pwr, phasor, mode=0, eps=eps)
                out.update(attrs=s_attractors, sep_pwr=s_sep_pwr, loss=loss, SNR=snr,
                           perm_idx=idx, perms=perms)
            if self.dpcl_weight is not None:
                # labels and weights from the CLEAN sources' magnitudes (forward_noisy included)
                out['loss'], out['dpcl'] = ops.dpcl_loss(s_embed_flat, fe['src_pwr'], out['loss'], self.dpcl_weight)
        if with_valid:
            if self.using_same_method and with_train:
                s_vattr, s_vsep = out['attrs'], out['sep_pwr']
            else:
                if self.valid_estimator.USE_TRUTH:
                    s_vattr = self.valid_estimator(
                        s_embed, s_src_pwr=fe['src_pwr'], s_mix_pwr=fe['mix_pwr'])
                else:
                    # main.py:267 passes only the embedding; the mixture magnitude is an
                    # extra keyword the reference's estimator signature already has
                    # (app/modules.py:501), used by the k-means extension as weights
                    s_vattr = self.valid_estimator(s_embed, s_mix_pwr=fe['mix_pwr'])
                s_vsep = self._separate(fe['mix_pwr'], s_vattr, s_embed_flat)  # :277-278
            vloss, perms, vidx, vsnr = ops.pit_mse_loss(       # main.py:312-313, 336-337
                s_src_signals, s_vsep, phasor, mode=1, eps=eps)
            out.update(valid_attrs=s_vattr, sep_pwr_valid=s_vsep, valid_loss=vloss,
                       valid_SNR=vsnr, valid_perm_idx=vidx, perms=perms)
        out['phasor'] = phasor
        out['mix_pwr'] = fe['mix_pwr']
        return out

    def forward_noisy(self, s_src_signals, s_noise, s_noise_gain=None, **kw):
        '''forward(s_src_signals, **kw) over a mixture with a component that is not a target (the wavdir dataset's
        NOISE_DIR): s_noise complex64 [B, T, F], s_noise_gain float32 [B] or None (= 1).  ops.noise_frontend
        replaces ops.frontend and nothing else changes: encoder, estimators, separator and loss see the noisy
        mixture, and the targets stay the CLEAN sources.  (A method of its own: forward() keeps its signature.)'''
        self._noise = (s_noise, s_noise_gain)
        try:
            return self.forward(s_src_signals, **kw)
        finally:
            self._noise = None

    def debug_fetch(self, s_src_signals):
        '''the `-m debug` fetch list (main.py:387-397): embed, attrs, input,
        output (+ module debug_fetches when hparams.DEBUG)'''
        with torch.no_grad():
            o = self.forward(s_src_signals)
            res = dict(embed=o['embed'], attrs=o['attrs'], input=s_src_signals,
                       output=ops.reattach_phase(o['sep_pwr'], o['phasor'], o['perm_idx']))
            for mod in (self.encoder, self.separator, self.estimator):
                res.update(getattr(mod, 'debug_fetches', {}) or {})
        return res

    # ------------------------------------------------------------ train step
    def train_step(self, s_src_signals, sync_metrics=True, s_noise=None, s_noise_gain=None):
        '''one `g_sess.run(train_fetches)` (main.py:430-431): forward, backward,
        gradient all-reduce, value clip, Adam.  Returns dict(loss, SNR, LR[, DPCL][, grad_norm, clip_coef]) of
        device scalars (no host sync unless the caller reads them).  s_noise / s_noise_gain: the step trains on
        the mixture of the sources and that noise against the clean sources (forward_noisy); None: today's step.'''
        # bounded run-ahead + status of the steps that have completed (raises DanetHipError
        # at most ops.MAX_STEPS_IN_FLIGHT steps after a hand-off timeout)
        ops.poll_status(self.device)
        if not self._grads_clean:
            self._flat_grad.zero_()
        chain = ops.heads_chain()        # small finalize kernels go to the side stream (ops.py)
        chain.__enter__()
        try:
            if s_noise is None:
                out = self.forward(s_src_signals, fuse_heads=self.fuse_heads,
                                   s_dropout_keep=float(hparams.DROPOUT_KEEP_PROB))    # main.py:429
            else:
                out = self.forward_noisy(s_src_signals, s_noise, s_noise_gain, fuse_heads=self.fuse_heads,
                                         s_dropout_keep=float(hparams.DROPOUT_KEEP_PROB))
        except BaseException:
            chain.__exit__(None, None, None)
            ops.drop_lazy(self.device)     # this step's queued finalizers must not run in the next
            raise
        self._early, self._in_step = None, True
        # from here until the final optimiser piece has been issued the bucket holds partial
        # sums: an exception in between (launch error, collective failure, KeyboardInterrupt)
        # must not leave it marked clean (fast_backward bypasses autograd's accumulate hook)
        self._grads_clean = False
        try:
            with ops.fast_backward():          # kernels add straight into the flat bucket
                out['loss'].backward(self._one)    # (a persistent 1: no ones_like fill per step)
                # side-stream finalizers (loss / SNR, anchor gradients) join the main stream
                # BEFORE the gradient reduction reads the bucket
                ops.join_deferred()
                if self._buckets is not None:
                    grad_scale = self._buckets.finish()            # pieces launched during backward
                else:                                              # ONE RCCL all-reduce / step
                    grad_scale = dist.allreduce_grads_(
                        self._grad_store if dist.is_dist() else self._flat_grad)
        finally:
            self._in_step = False
            chain.__exit__(None, None, None)
            ops.join_deferred()        # (no-op after a clean backward; an exception path still joins)
        self.step_count += 1
        ranges, early_stream = None, None
        if self._early is not None:            # everything but the bottom layer is already stepped
            early, early_stream = self._early
            ranges = dist._complement(early, self._flat_grad.numel())
            self._early = None
        norm_out = None
        if self.grad_clip_norm is None:
            self.ozer.step(self.step_count, self.learn_rate, clip=hparams.GRAD_CLIP_THRES,
                           grad_scale=grad_scale, zero_grad=not self.keep_grads, ranges=ranges)
        else:
            # the gradients alone: the 4 status words in front of the store are no part of the norm.  The partials
            # are this model's, written and read on this stream every step; (norm, coef) is a NEW tensor every
            # step, because the caller may keep the returned scalars over many steps (feed.StepReport)
            self._gclip_partials = ops.grad_sumsq(self._flat_grad, self._gclip_partials)
            norm_out = torch.empty(2, dtype=torch.float64, device=self.device)
            self.ozer.step(self.step_count, self.learn_rate, clip=hparams.GRAD_CLIP_THRES,
                           grad_scale=grad_scale, zero_grad=not self.keep_grads, max_norm=self.grad_clip_norm,
                           partials=self._gclip_partials, norm_out=norm_out)
        ops.repack_weights(self.device)    # operand-layout copies of the weights the GEMMs read
        if early_stream is not None:
            # joined AFTER the last piece (disjoint ranges): by now the early piece has long
            # finished, and a wait for an already signalled event costs nothing (waiting first
            # put a 20 us bubble in front of the last kernel of the step)
            torch.cuda.current_stream(self.device).wait_stream(early_stream)
        self._grads_clean = not self.keep_grads
        ops.step_done(self.device)
        if self._auto:
            self._auto_tick()
        res = dict(loss=out['loss'].detach(), SNR=out['SNR'], LR=self.learn_rate)
        if self.dpcl_weight is not None:
            res['DPCL'] = out['dpcl']
        if norm_out is not None:
            res.update(grad_norm=norm_out[0], clip_coef=norm_out[1])
        return res

    def collectives_per_step(self):
        '''data-path collectives a train step issues under data parallelism (0 without)'''
        if not dist.is_dist():
            return 0
        return {'0': 1, 'tail': 2}.get(self.grad_schedule,
                                       1 + hparams.NUM_LSTM_LAYERS + 1)   # '1': per-layer buckets

    def valid_step(self, s_src_signals, s_noise=None, s_noise_gain=None):
        '''`g_sess.run(valid_fetches)` (main.py:499-500).  s_noise / s_noise_gain (the wavdir dataset's
        NOISE_EVAL_DIR): the step evaluates the mixture of the sources and that noise against the clean sources
        (forward_noisy) -- `loss` and `SNR` are the reference's validation loss of the noisy mixture, and with
        EVAL_SI_SDR true `SI-SDR`, `SI-SDRi` (against the noisy mixture the model was given) and `nSNR` (sources to
        noise, dB) come from ops.si_sdr_noisy; None: today's step.'''
        ops.poll_status(self.device)
        if s_noise is not None:
            with torch.no_grad():
                out = self.forward_noisy(s_src_signals, s_noise, s_noise_gain, with_valid=True, with_train=False)
                res = dict(loss=out['valid_loss'], SNR=out['valid_SNR'])
                if self.eval_si_sdr:
                    est = ops.reattach_phase(out['sep_pwr_valid'], out['phasor'])
                    res['SI-SDR'], res['SI-SDRi'], res['nSNR'] = ops.si_sdr_noisy(
                        s_src_signals, est, s_noise, s_noise_gain)[:3]
            ops.step_done(self.device, collective_consistent=not dist.is_dist())
            return res
        with torch.no_grad():
            out = self.forward(s_src_signals, with_valid=True, with_train=False)
            res = dict(loss=out['valid_loss'], SNR=out['valid_SNR'])
            wav = None
            if self.eval_si_sdr:
                # the waveform metric does its own permutation search: the estimates go in unpermuted
                est = self._refined(ops.reattach_phase(out['sep_pwr_valid'], out['phasor']), s_src_signals)
                if self.eval_bss is None and not self.eval_stoi:
                    res['SI-SDR'], res['SI-SDRi'] = ops.si_sdr(s_src_signals, est)[:2]
                else:
                    res['SI-SDR'], res['SI-SDRi'], _, _, wav = ops.si_sdr_wav(s_src_signals, est)
            elif self.eval_bss is not None or self.eval_stoi:
                est = self._refined(ops.reattach_phase(out['sep_pwr_valid'], out['phasor']), s_src_signals)
                if self.eval_bss is not None and self.eval_stoi:
                    # both read the waveforms: synthesised once, into the metric's cached scratch
                    wav = ops.synth_wav(s_src_signals, est)
            if self.eval_bss is not None:
                # BSS-eval on the same waveforms (synthesised once); its permutation is its own too
                res['SDR'], res['SIR'], res['SAR'], res['SDRi'] = ops.bss_eval(
                    s_src_signals, est, self.eval_bss, wav=wav)[:4]
            if self.eval_stoi:
                res['STOI'], res['ESTOI'], res['STOIi'], res['ESTOIi'] = ops.stoi_eval(s_src_signals, est, wav=wav)[:4]
        ops.step_done(self.device, collective_consistent=not dist.is_dist())
        return res

    def _refined(self, est, mixrows):
        '''est complex64 [B, C, T, F] after PHASE_REFINE_ITERS iterations of MISI against the mixture that is the sum
        of mixrows [B, Cm, T, F]; est itself with the key null'''
        if self.phase_refine is None:
            return est
        return ops.phase_refine(est, mixrows, self.phase_refine)

    def infer(self, s_mixed_signals):
        '''`g_sess.run(infer_fetches, {s_mixed_signals: ...})` (main.py:384-385,
        685-690): complex mixture [B,T,F] -> separated complex [B,C,T,F] using
        the inference estimator and the mixture phase (main.py:333-335); with PHASE_REFINE_ITERS set, that phase
        refined by ops.phase_refine.'''
        if self.stream_block is not None:
            return self._infer_stream(s_mixed_signals)
        if self.infer_chunk is not None:
            if s_mixed_signals.shape[0] != 1:
                raise ValueError('INFER_CHUNK_LEN is set: infer takes one recording at a time (got a batch of %d)'
                                 % s_mixed_signals.shape[0])
            if s_mixed_signals.shape[1] > self.infer_chunk[0]:
                return self.infer_long(s_mixed_signals)
        B, E = hparams.BATCH_SIZE, hparams.EMBED_SIZE
        ops.poll_status(self.device)
        with torch.no_grad():
            fe = ops.frontend(s_mixed_signals[:, None].contiguous())
            s_embed = self.encoder(fe['mix_log'])
            s_attr = self.valid_estimator(s_embed, s_mix_pwr=fe['mix_pwr'])
            s_sep = self._separate(fe['mix_pwr'], s_attr, s_embed.reshape(B, -1, E))
            res = self._refined(ops.reattach_phase(s_sep, fe['phasor']), s_mixed_signals[:, None])
        ops.step_done(self.device, collective_consistent=not dist.is_dist())
        return res

    def _infer_stream(self, s_mixed_signals):
        '''infer with INFER_STREAM_BLOCK = n: the recording goes through a stream session in blocks of n frames and the
        separated blocks are concatenated; bit for bit what any other block size gives'''
        if hparams.BATCH_SIZE > ops.CAUSAL_MAX_B:
            raise ValueError('INFER_STREAM_BLOCK needs BATCH_SIZE <= %d when infer runs (got %d)'
                             % (ops.CAUSAL_MAX_B, hparams.BATCH_SIZE))
        n, T = self.stream_block, s_mixed_signals.shape[1]
        ops.poll_status(self.device)
        stream = self.open_stream(s_mixed_signals.shape[0])
        parts = [stream.push(s_mixed_signals[:, t:t + n]) for t in range(0, T, n)]
        parts.append(stream.flush())
        ops.step_done(self.device, collective_consistent=not dist.is_dist())
        return torch.cat(parts, dim=2)

    def infer_chunks(self, s_chunks):
        '''the chunks of one recording, complex64 [n, L, F] -> (mags float32 [n, C, L, F], phasor float32
        [n, L, F, 2]): the separated magnitudes of every chunk BEFORE phase re-attachment, channels in each chunk's own
        order, and the mixture phasor.  The chunks go through infer's front-end, encoder, inference estimator and
        separator in groups of INFER_CHUNK_BATCH; the plugins reshape by hparams.BATCH_SIZE, which is the group's size
        for the duration of the group.  A group size the recurrent kernels refuse surfaces their error unchanged.'''
        G = self.infer_chunk[2] if self.infer_chunk is not None else 16
        n, L, F = s_chunks.shape
        C, E = hparams.MAX_N_SIGNAL, hparams.EMBED_SIZE
        mags = torch.empty(n, C, L, F, device=self.device)
        phasor = torch.empty(n, L, F, 2, device=self.device)
        ops.poll_status(self.device)
        batch_size = hparams.BATCH_SIZE
        try:
            with torch.no_grad():
                for g0 in range(0, n, G):
                    g = min(G, n - g0)
                    hparams.BATCH_SIZE = g
                    fe = ops.frontend(s_chunks[g0:g0 + g, None].contiguous())
                    s_embed = self.encoder(fe['mix_log'])
                    s_attr = self.valid_estimator(s_embed, s_mix_pwr=fe['mix_pwr'])
                    mags[g0:g0 + g] = self.separator(fe['mix_pwr'], s_attr, s_embed.reshape(g, -1, E))
                    phasor[g0:g0 + g] = fe['phasor']
        finally:
            hparams.BATCH_SIZE = batch_size
        ops.step_done(self.device, collective_consistent=not dist.is_dist())
        return mags, phasor

    def infer_long(self, s_mixed_signals):
        '''infer for a recording longer than one chunk, complex64 [1, T, F] -> [1, C, T, F]: the plan of
        include/danet_stitch_hip.h cuts it into overlapping chunks (plain tensor slicing), infer_chunks separates them
        and ops.stitch aligns their channels, cross-fades the overlaps and re-attaches the mixture phase'''
        L, V, _G = self.infer_chunk
        T = s_mixed_signals.shape[1]
        assert s_mixed_signals.shape[0] == 1 and T > L, s_mixed_signals.shape
        starts = ops.stitch_plan(T, L, V)
        s_chunks = torch.stack([s_mixed_signals[0, s:s + L] for s in starts])
        mags, phasor = self.infer_chunks(s_chunks)
        # the stitched recording is refined as a whole, against the whole mixture: T frames, one call
        return self._refined(ops.stitch(mags, phasor, T, V)[None], s_mixed_signals[:, None])

    # ------------------------------------------------------- misc (main.py)
    def set_learn_rate(self, lr):
        self.learn_rate = float(lr)

    def get_learn_rate(self):
        return self.learn_rate

    def check_status(self):
        '''blocking check of the persistent kernels' hand-off status (end of an epoch / a
        sweep, before parameters or separated signals are written); raises DanetHipError
        after a timeout -- on every rank together under data parallelism'''
        ops.check_status(self.device)

    def status_words(self):
        '''the 4 spare floats of the gradient store (word 0 = hand-off status under data parallelism)'''
        return self._grad_store[:4]

    def zero_grad(self):
        self._flat_grad.zero_()
        self._grads_clean = True

    def reset_state(self):
        '''RNN states are never carried (main.py:538-540 re-zeros zeros)'''
        return

    def save_params(self, filename, step=None):
        '''trainable variables only, like tf.train.Saver(var_list=trainables)
        (main.py:357,399); stored as .npz keyed by the reference's TF variable
        names (a TF1 checkpoint cannot be written without TF).  One extra entry, `step_count`:
        the number of train steps taken (over all resumed runs), which is also the `step` word of the dropout masks --
        a run resumed from the file continues the mask sequence.'''
        save_dir = os.path.dirname(os.path.abspath(filename))
        if not os.path.exists(save_dir):
            os.makedirs(save_dir)
        if step is not None:
            filename = '%s-%d' % (filename, step)
        np.savez(filename, step_count=np.int64(self.step_base + self.step_count),
                 **{k: v.detach().cpu().numpy() for k, v in self.vars.items()})

    def load_params(self, filename):
        if not filename.endswith('.npz'):
            filename = filename + '.npz'
        data = np.load(filename)
        with torch.no_grad():
            for k, v in self.vars.items():
                v.copy_(torch.as_tensor(data[k]).to(self.device))
        if 'step_count' in data.files:       # (files written before the entry existed: unchanged)
            self.step_base = int(data['step_count']) - self.step_count
        return True

    def weights_written(self):
        '''REQUIRED after any write to the parameters that torch's version counter does not see
        (`param.data` arithmetic, c10d collectives, an external optimizer or kernel writing
        through raw pointers): marks the operand-layout copies of the weights (ops.packed_weight,
        read by the projection / dYc / dX / gx products) stale, so the next product re-packs them.
        In-place torch ops on the variables themselves and this package's own optimizer step need
        no call.'''
        ops.weights_written(self._flat)

    def load_param_dict(self, di):
        '''set variables from {tf_variable_name: ndarray} (tests / oracle parity)'''
        with torch.no_grad():
            for k, a in di.items():
                self.vars[k].copy_(torch.as_tensor(np.asarray(a, dtype=np.float32)).to(self.device))

    def param_dict(self):
        return {k: v.detach().cpu().numpy() for k, v in self.vars.items()}

    def grad_dict(self):
        return {k: v.grad.detach().cpu().numpy() for k, v in self.vars.items()}


class SeparationStream(object):
    '''Block-wise streaming inference (Model.open_stream): push(frames) takes the next frames of `batch` recordings,
    complex64 [batch, n, F], and returns the separated frames the call decided, complex64 [batch, C, m, F].  The
    session owns everything that travels from block to block -- the two centring states, the LSTM layers' h and c, the
    online estimator's state and the absolute frame index -- and runs each block of at most 64 frames through
    ops.frontend, the causal centring, ops.causal_lstm_block, the causal centring, ops.causal_project, ops.online_scan,
    ops.online_separate and ops.reattach_phase (include/danet_causal_hip.h, include/danet_online_hip.h).  Every one of
    them gives a frame the same bits whatever block it arrives in, so the concatenated output does not depend on how
    the recording was cut.

    Until T0 = ONLINE_INIT_FRAMES frames have arrived their embedding and |mix| are kept and push returns zero
    frames (the online estimator forms A0 from the first T0 frames); the call that brings frame T0 - 1 returns every
    frame so far.  flush() ends the recording: past the hold it has nothing left to return; on a recording no longer
    than the hold it returns what Model.infer returns there, the plain separator with A0 of the frames there are.
    reset() starts the next recording.  The STFT is per frame and stays with the caller, as with Model.infer.'''

    BLOCK = ops.CAUSAL_MAX_TB

    def __init__(self, model, batch=1):
        Model._check_stream_model('open_stream')
        if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= ops.CAUSAL_MAX_B:
            raise ValueError('open_stream: batch must be an integer in 1..%d (got %r); BATCH_SIZE recordings at most '
                             'that many go through one session' % (ops.CAUSAL_MAX_B, batch))
        if not model.built or model.online is None:
            raise ValueError('open_stream needs a built model with INFER_ESTIMATOR_METHOD = "online"')
        self.model, self.batch = model, batch
        H, L = model.encoder._dims()
        if H % 4 or H > ops.CAUSAL_MAX_H or L > ops.CAUSAL_MAX_L or hparams.FEATURE_SIZE > ops.CAUSAL_MAX_D0:
            raise ValueError('open_stream needs LSTM_HDIM a multiple of 4 and <= %d, NUM_LSTM_LAYERS <= %d and FFT_SIZE '
                             '<= %d (got %d, %d, %d)' % (ops.CAUSAL_MAX_H, ops.CAUSAL_MAX_L,
                                                         2 * (ops.CAUSAL_MAX_D0 - 1), H, L, hparams.FFT_SIZE))
        self.H, self.L = H, L
        enc = 'global/' + model.encoder.name
        # (views into the model's flat parameter buffer.  danet_causal_lstm_block wants W[l] 16-byte aligned: they are,
        # because the encoder's variables come first in that buffer and each holds a multiple of 4 floats when H % 4 == 0;
        # a layout that broke this would be refused by the library with a message, not read misaligned)
        self.Ws =[model.vars['%s/lstm%d/LSTM/linear/W' % (enc, l)].detach() for l in range(L)]
        self.bs = [model.vars['%s/lstm%d/LSTM/linear/B' % (enc, l)].detach() for l in range(L)]
        self.Wout = model.vars[enc + '/output/W'].detach()
        self.anchors = model.vars['global/%s/anchors' % model.valid_estimator.name].detach()
        dev = model.device
        self.h = torch.empty(L, batch, H, device=dev)
        self.c = torch.empty(L, batch, H, device=dev)
        self.center_in = ops.causal_center_state(batch, dev)
        self.center_top = ops.causal_center_state(batch, dev)
        # what a block needs between its launches, owned here and sized for BLOCK frames so that push allocates only
        # what it returns or keeps: the centred input, the top layer's output, its centred copy, the block kernel's
        # workspace.  Every launch is ordered on the stream, so the next block may overwrite them.
        self.Fp = (hparams.FEATURE_SIZE + 3) // 4 * 4
        self.xc = torch.empty(self.BLOCK * batch * self.Fp, device=dev)
        self.y = torch.empty(self.BLOCK * batch * H, device=dev)
        self.yc = torch.empty(self.BLOCK * batch * H, device=dev)
        self.ws = torch.empty(ops.causal_lstm_ws_bytes(L, batch, self.BLOCK, H) // 4, device=dev)
        # the embedding [batch, n, F, E] of the last block and the attractors [batch, m, C, E] of the last frames
        # decided (tests and tools)
        self.embed = self.attr = None
        self.reset()

    def reset(self):
        '''forget the recording: zero state, frame index 0'''
        for t in (self.h, self.c, self.center_in, self.center_top):
            t.zero_()
        self.t = 0                   # the absolute index of the next frame
        self.state = None            # the online estimator's state, float64 [batch, 2 C E + C], once A0 exists
        self.held = []               # (embed, mix_pwr, phasor) of the blocks of the hold

    def _encode(self, frames):
        '''the next n <= 64 frames -> (embed [batch, n, F, E], mix_pwr [batch, n, F], phasor [batch, n, F, 2])'''
        B, n, F = frames.shape
        E, H, Fp = hparams.EMBED_SIZE, self.H, self.Fp
        fe = ops.frontend(frames[:, None].contiguous())
        xc = self.xc[:n * B * Fp].view(n, B, Fp)
        y = self.y[:n * B * H].view(n, B, H)
        yc = self.yc[:B * n * H].view(B, n, H)
        ops.causal_center_fwd(fe['mix_log'], B, n, F, 0, F, xc, 1, Fp, self.center_in)
        ops.causal_lstm_block(xc, Fp, F, self.Ws, self.bs, self.h, self.c, y=y, ldy=H, ws=self.ws)
        ops.causal_center_fwd(y, B, n, H, 1, H, yc, 0, H, self.center_top)
        embed = ops.causal_project(yc, B * n, H, F * E, H, self.Wout, F * E).view(B, n, F, E)
        return embed, fe['mix_pwr'], fe['phasor']

    def _track(self, embed, w, phasor, t_first):
        '''the online estimator over the frames t_first .. of the recording, from the carried state'''
        m = self.model
        T0, lam = m.online
        attr = ops.online_scan(embed, w, self.state, m.separator.ACT, lam, T0, float(hparams.EPS), t_first=t_first)
        self.attr = attr
        return ops.reattach_phase(ops.online_separate(w, attr, embed, m.separator.ACT), phasor)

    def _empty(self):
        return torch.empty(self.batch, hparams.MAX_N_SIGNAL, 0, hparams.FEATURE_SIZE, dtype=torch.complex64,
                           device=self.model.device)

    def _a0(self):
        '''(A0 [batch, C, E] of the first min(T0, frames held) frames, and the held frames joined)'''
        embed, w, phasor = (torch.cat(parts, dim=1) for parts in zip(*self.held))
        T0 = self.model.online[0]
        a0, _, _ = ops.AnchorAttractorFn.apply(embed[:, :T0].contiguous(), self.anchors, hparams.MAX_N_SIGNAL)
        return a0, embed, w, phasor

    def _block(self, frames):
        embed, w, phasor = self._encode(frames)
        self.embed = embed
        t_first, self.t = self.t, self.t + frames.shape[1]
        if self.state is not None:
            return self._track(embed, w, phasor, t_first)
        self.held.append((embed, w, phasor))
        if self.t < self.model.online[0]:
            return self._empty()
        a0, embed, w, phasor = self._a0()
        self.held = []
        self.state = ops.online_init(a0)
        return self._track(embed.contiguous(), w.contiguous(), phasor.contiguous(), 0)

    def push(self, frames):
        '''the next n >= 0 frames of every recording, complex64 [batch, n, F] -> the m frames this call decided,
        complex64 [batch, C, m, F]'''
        if frames.dim() != 3 or frames.shape[0] != self.batch or frames.shape[2] != hparams.FEATURE_SIZE \
                or frames.dtype != torch.complex64:
            raise ValueError('push takes complex64 [batch = %d, n, F = %d] (got %s %s)'
                             % (self.batch, hparams.FEATURE_SIZE, frames.dtype, tuple(frames.shape)))
        with torch.no_grad():
            parts = [self._block(frames[:, s:s + self.BLOCK]) for s in range(0, frames.shape[1], self.BLOCK)]
            return torch.cat(parts, dim=2) if parts else self._empty()

    def flush(self):
        '''end the recording: the frames still held (a recording no longer than the hold: the plain separator with A0
        of the frames there are, as Model.infer there), else zero frames; then reset()'''
        with torch.no_grad():
            out = self._empty()
            if self.held:
                a0, embed, w, phasor = self._a0()
                sep = self.model.separator(w, a0, embed.reshape(self.batch, -1, hparams.EMBED_SIZE))
                out = ops.reattach_phase(sep, phasor.contiguous())
        self.reset()
        return out
