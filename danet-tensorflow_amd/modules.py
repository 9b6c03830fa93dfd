'''
Encoder / Estimator / Separator plugins -- the drop-in boundary.

Same class hierarchy, constructor signature `(model, name)`, `__call__`
signatures, `USE_TRUTH` flags, `debug_fetches` behaviour and
`@hparams.register_*` names as the reference's `app/modules.py:11-603`, so
`hparams.get_encoder()` / `get_estimator(name)` / `get_separator(name)` resolve
to MI355X-native implementations unchanged.  Tensors are eager torch CUDA
tensors instead of TF symbolic tensors; every `__call__` runs hand-written HIP
kernels through `ops` (no CPU fallback).

Extension (defaults = the reference's hard-coded values, app/modules.py:153,
212,223-242): `hparams.NUM_LSTM_LAYERS`, `hparams.LSTM_HDIM`.  The `conv-bilstm-v1`
encoder's convolutions run on the extension library libdanet_conv_hip.so; the BiLSTM
encoders' dropout (`s_dropout_keep` < 1) on libdanet_dropout_hip.so.
'''
from math import sqrt

import numpy as np
import torch

from .hparams import hparams
from . import ops


class ModelModule(object):
    '''abstract sub-module of model (app/modules.py:11-25)'''
    def __init__(self, model, name):
        if hparams.DEBUG:
            self.debug_fetches = {}
        self.name = name
        self.model = model

    def __call__(self, s_dropout_keep=1.):
        raise NotImplementedError()


class Encoder(ModelModule):
    '''maps log-magnitude-spectra to embedding (app/modules.py:28-50)'''
    def __init__(self, model, name):
        super(Encoder, self).__init__(model, name)

    def __call__(self, s_mixture, s_dropout_keep=1.):
        '''[batch_size, length, feature_size] ->
        [batch_size, length, feature_size, embedding_size]'''
        raise NotImplementedError()


class Estimator(ModelModule):
    '''Estimates attractor location (app/modules.py:53-70)'''
    USE_TRUTH = True

    def __init__(self, model, name):
        super(Estimator, self).__init__(model, name)

    def __call__(self, s_embed, **kwargs):
        '''[B, T, F, E] -> [B, num_signals, E]'''
        raise NotImplementedError()


class Separator(ModelModule):
    '''mixture magnitudes + attractors + embedding -> separated magnitudes
    (app/modules.py:73-93)'''
    def __init__(self, model, name):
        super(Separator, self).__init__(model, name)

    def __call__(self, s_mixed_signals_pwr, s_attractors, s_embed_flat):
        raise NotImplementedError()


def _uniform_init(r):
    def init(shape, gen):
        return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).mul_(r).float()
    return init


def _const_init(arr):
    def init(shape, gen):
        return torch.as_tensor(np.asarray(arr, dtype=np.float32)).reshape(shape).clone()
    return init


def _lstm_bias(hdim, i_bias=1.5):
    b = np.zeros([hdim * 4], dtype=np.float32)
    b[hdim * 1:hdim * 2] = i_bias   # input gate   (modules.py:218)
    b[hdim * 2:hdim * 3] = -1.      # forget gate  (modules.py:219)
    b[hdim * 3:hdim * 4] = 1.       # output gate  (modules.py:220)
    return b


@hparams.register_encoder('toy')
class ToyEncoder(Encoder):
    '''2-layer MLP for debugging (app/modules.py:96-116); s_dropout_keep is accepted and ignored,
    as in the reference'''
    def __init__(self, model, name):
        super(ToyEncoder, self).__init__(model, name)

    def __call__(self, s_signals, s_dropout_keep=1.):
        F, E = hparams.FEATURE_SIZE, hparams.EMBED_SIZE
        m = self.model
        hid = hparams.FFT_SIZE * 2
        # TF default initialiser for get_variable is glorot_uniform
        w0 = m.get_variable(self.name + '/linear0/W', [F, hid],
                            _uniform_init(sqrt(6. / (F + hid))))
        b0 = m.get_variable(self.name + '/linear0/B', [hid], _const_init(np.zeros(hid)))
        w1 = m.get_variable(self.name + '/linear1/W', [hid, F * E],
                            _uniform_init(sqrt(6. / (hid + F * E))))
        b1 = m.get_variable(self.name + '/linear1/B', [F * E], _const_init(np.zeros(F * E)))
        s_mid = ops.lyr_linear(s_signals, w0, b0)
        s_mid = ops.relu(s_mid, hparams.RELU_LEAKAGE)
        s_out = ops.lyr_linear(s_mid, w1, b1)
        return s_out.reshape(hparams.BATCH_SIZE, -1, F, E)


def _lyr_bilstm(name_, model_, s_input_, hdim_, t_axis_, axis_, w_init_, b_init_,
                s_dropout_keep_):
    '''one bidirectional layer on a batch-major tensor (app/modules.py:120-137);
    fwd and reversed-bwd scans run concurrently in one persistent launch, then
    `tf.nn.dropout(s_output, keep_prob)` (app/modules.py:137) as inverted dropout on
    libdanet_dropout_hip.so when s_dropout_keep_ < 1 (the mask: `model_.dropout_spec`,
    one stream id per call in call order).  With keep 1 there is no dropout launch.'''
    assert t_axis_ in (-2, 1) and axis_ in (-1, 2)
    D = s_input_.shape[-1]
    params = []
    for d in ('_fwd', '_bwd'):
        W = model_.get_variable('%s%s/LSTM/linear/W' % (name_, d), [D + hdim_, 4 * hdim_], w_init_)
        b = model_.get_variable('%s%s/LSTM/linear/B' % (name_, d), [4 * hdim_], b_init_)
        params += [W, b]
    with ops.dropout_scope(_dropout_spec(model_, s_dropout_keep_)):
        return ops.LstmLayerFn.apply(s_input_, hdim_, *params)


def _dropout_spec(model, keep):
    '''the step's ops.DropoutSpec for keep < 1 (Model.dropout_spec: seed, rank, step), else None'''
    return model.dropout_spec(keep) if float(keep) < 1. else None


class _RnnEncoderBase(Encoder):
    NDIR = 1
    INIT_SCALE = 1.15

    def _dims(self):
        raise NotImplementedError()

    def __call__(self, s_signals, s_dropout_keep=1.):
        hdim, nlayer = self._dims()
        F, E = hparams.FEATURE_SIZE, hparams.EMBED_SIZE
        m = self.model
        init_range = self.INIT_SCALE / sqrt(hdim)           # modules.py:154 / :213
        w_initer = _uniform_init(init_range)
        b_initer = _const_init(_lstm_bias(hdim))            # modules.py:158-162 / :217-221
        params = []
        D = F
        for l in range(nlayer):
            for d in (('_fwd', '_bwd') if self.NDIR == 2 else ('',)):
                base = '%s/lstm%d%s/LSTM/linear/' % (self.name, l, d)
                params.append(m.get_variable(base + 'W', [D + hdim, 4 * hdim], w_initer))
                params.append(m.get_variable(base + 'B', [4 * hdim], b_initer))
            D = self.NDIR * hdim
        params.append(m.get_variable(self.name + '/output/W', [D, F * E],
                                     _uniform_init(1.85)))  # modules.py:184-191 / :248-255
        s_out = self._encode(s_signals, hdim, nlayer, params, s_dropout_keep)
        return s_out.reshape(hparams.BATCH_SIZE, -1, F, E)  # modules.py:192-195 / :256-259

    def _encode(self, s_signals, hdim, nlayer, params, s_dropout_keep):
        # (NDIR == 1, `lstm-orig`: accepted and ignored, as in the reference's class)
        with ops.dropout_scope(_dropout_spec(self.model, s_dropout_keep) if self.NDIR == 2 else None):
            return ops.RnnEncoderFn.apply(s_signals, hdim, nlayer, self.NDIR, *params)


@hparams.register_encoder('lstm-orig')
class LstmEncoder(_RnnEncoderBase):
    '''unidirectional LSTM stack as in the original paper (app/modules.py:140-196);
    reference shape 4 x 600.  s_dropout_keep is accepted and ignored: the reference builds this
    stack from model.lyr_lstm, which has no dropout'''
    NDIR = 1
    INIT_SCALE = 1.15

    def __init__(self, model, name):
        super(LstmEncoder, self).__init__(model, name)

    def _dims(self):
        # the reference hard-codes 600 units for the unidirectional stack
        # (modules.py:153); LSTM_HDIM's default (300) is the BiLSTM width, so
        # only a non-default value overrides it.
        h = hparams.LSTM_HDIM
        return (600 if h == 300 else h), hparams.NUM_LSTM_LAYERS


@hparams.register_encoder('lstm-causal')
class LstmCausalEncoder(LstmEncoder):
    '''the `lstm-orig` stack with both whole-utterance centrings replaced by the running mean over the frames seen so
    far (include/danet_causal_hip.h): the embedding of frame t depends on frames <= t only.  NOT in the reference.
    Same variable names, shapes, initialisers, creation order and `_dims()` as `lstm-orig`, so its parameter files
    load; it trains on the same recurrent kernels (ops.CausalRnnEncoderFn), and Model.open_stream runs it block by
    block from carried state.  s_dropout_keep is accepted and ignored, as in `lstm-orig`.'''

    def _encode(self, s_signals, hdim, nlayer, params, s_dropout_keep):
        return ops.CausalRnnEncoderFn.apply(s_signals, hdim, nlayer, *params)


@hparams.register_encoder('bilstm-orig')
class BiLstmEncoder(_RnnEncoderBase):
    '''Bi-LSTM stack as in the original paper (app/modules.py:199-260);
    reference shape 4 x 300 per direction'''
    NDIR = 2
    INIT_SCALE = .75

    def __init__(self, model, name):
        super(BiLstmEncoder, self).__init__(model, name)

    def _dims(self):
        return hparams.LSTM_HDIM, hparams.NUM_LSTM_LAYERS


@hparams.register_encoder('conv-bilstm-v1')
class ConvBiLstmEncoder(Encoder):
    '''Experimental CNN-LSTM hybrid network (app/modules.py:263-379): 8 conv layers (2-D
    convolution, max-pooling and depth-to-space on libdanet_conv_hip.so) around a 2-layer BiLSTM of
    width FFT_SIZE with a centred residual, then a bias-free dense layer.  The LSTM width and depth
    are the reference's (FFT_SIZE, 2) whatever LSTM_HDIM / NUM_LSTM_LAYERS say; the number of frames
    must be a multiple of 4 (LENGTH_ALIGN) and FFT_SIZE a multiple of 8, >= 16.'''
    def __init__(self, model, name):
        super(ConvBiLstmEncoder, self).__init__(model, name)

    def _conv_vars(self, scope, k, cin, cout, w_init=None):
        # tf.layers.conv2d: kernel [k, k, Cin, Cout] (glorot-uniform unless given), bias zeros
        if w_init is None:
            w_init = _uniform_init(sqrt(6. / (k * k * (cin + cout))))
        m = self.model
        w = m.get_variable('%s/%s/kernel' % (self.name, scope), [k, k, cin, cout], w_init)
        b = m.get_variable('%s/%s/bias' % (self.name, scope), [cout], _const_init(np.zeros(cout)))
        return [w, b]

    def __call__(self, s_signals, s_dropout_keep=1.):
        B, T, F = s_signals.shape
        nfft, E = hparams.FFT_SIZE, hparams.EMBED_SIZE
        ops.conv_encoder_check(T, nfft, F)
        m = self.model
        w_initer = _uniform_init(2. / sqrt(nfft))                     # modules.py:278-280
        b_initer = _const_init(_lstm_bias(nfft, i_bias=1.))           # modules.py:282-287
        conv_w_initer = _uniform_init(3e-1)                            # modules.py:336-338
        names = ['conv2d'] + ['conv2d_%d' % i for i in range(1, 8)]
        params = []
        for i, (cin, cout, k, _, _) in enumerate(ops.CONV_LAYERS[:4]):
            params += self._conv_vars(names[i], k, cin, cout)
        for l in range(2):
            for d in ('_fwd', '_bwd'):
                base = '%s/lstm%d%s/LSTM/linear/' % (self.name, l, d)
                params.append(m.get_variable(base + 'W', [2 * nfft + nfft, 4 * nfft], w_initer))
                params.append(m.get_variable(base + 'B', [4 * nfft], b_initer))
        for i, (cin, cout, k, _, _) in enumerate(ops.CONV_LAYERS[4:], 4):
            params += self._conv_vars(names[i], k, cin, cout, conv_w_initer if i < 6 else None)
        O = F * E
        params.append(m.get_variable(self.name + '/dense/kernel', [nfft, O],
                                     _uniform_init(sqrt(6. / (nfft + O)))))
        debug = {} if hparams.DEBUG else None
        with ops.dropout_scope(_dropout_spec(m, s_dropout_keep)):
            s_out = ops.ConvBiLstmEncoderFn.apply(s_signals, nfft, float(hparams.RELU_LEAKAGE), debug, *params)
        if hparams.DEBUG:
            # the reference's NCHW shapes (copies: debug path only)
            T4, N8 = T // 4, nfft // 8
            nchw = lambda t: t.detach().view(T4, B, 16, N8).permute(1, 2, 0, 3).contiguous()
            self.debug_fetches = dict(conv_act=nchw(debug['conv_act']), lstm_act=nchw(debug['lstm_act']),
                                      mid4=debug['mid4'].detach().clone())
        return s_out.reshape(hparams.BATCH_SIZE, -1, F, E)            # modules.py:372-374


class _TruthEstimatorBase(Estimator):
    USE_TRUTH = True
    MODE = None

    def __call__(self, s_embed, s_src_pwr, s_mix_pwr, s_embed_flat=None):
        s_attractors = ops.TruthAttractorFn.apply(
            s_embed, s_src_pwr, s_mix_pwr, ops.TRUTH_MODES[self.MODE], float(hparams.EPS))
        if hparams.DEBUG:
            self.debug_fetches = dict()
        return s_attractors                                  # float[B, C, E]


@hparams.register_estimator('truth')
class AverageEstimator(_TruthEstimatorBase):
    '''simple average of true assignment (app/modules.py:382-412)'''
    MODE = 'truth'

    def __init__(self, model, name):
        super(AverageEstimator, self).__init__(model, name)


@hparams.register_estimator('truth-threshold')
class ThreshouldedAverageEstimator(_TruthEstimatorBase):
    '''true assignment, bins with |mix| <= 5 cut (app/modules.py:415-450)'''
    MODE = 'truth-threshold'

    def __init__(self, model, name):
        super(ThreshouldedAverageEstimator, self).__init__(model, name)


@hparams.register_estimator('truth-weighted')
class WeightedAverageEstimator(_TruthEstimatorBase):
    '''|mix|-weighted average of true assignment (app/modules.py:453-487)'''
    MODE = 'truth-weighted'

    def __init__(self, model, name):
        super(WeightedAverageEstimator, self).__init__(model, name)


@hparams.register_estimator('anchor')
class AnchoredEstimator(Estimator):
    '''best anchor subset + one EM step (app/modules.py:490-545)'''
    USE_TRUTH = False

    def __init__(self, model, name):
        super(AnchoredEstimator, self).__init__(model, name)
        self.name = name

    def __call__(self, s_embed, s_src_pwr=None, s_mix_pwr=None, s_embed_flat=None):
        v_anchors = self.model.get_variable(
            self.name + '/anchors', [hparams.NUM_ANCHOR, hparams.EMBED_SIZE],
            lambda shape, gen: torch.randn(shape, generator=gen, dtype=torch.float64).float())
        s_attractors, s_attractor_sets, s_subset_choice = ops.AnchorAttractorFn.apply(
            s_embed, v_anchors, hparams.MAX_N_SIGNAL)
        if hparams.DEBUG:
            self.debug_fetches = dict(
                asets=s_attractor_sets, anchors=v_anchors, subset_choice=s_subset_choice)
        return s_attractors


@hparams.register_estimator('kmeans')
class KMeansEstimator(Estimator):
    '''k-means-style attractor estimation for inference (BASELINE cfg 5).  NOT in
    the reference ("Only the favorable anchor method is implemented",
    README.md:216) -- an extension with no reference behaviour to match.
    Initialised from the anchor estimator's attractors (so it shares the
    `anchors` variable name and shape, app/modules.py:503-506), then
    hparams.KMEANS_ITERS Lloyd iterations: assign every time-frequency bin to its
    nearest attractor by dot product (the separator's own similarity), recompute
    each attractor as the |mix|-weighted mean of its bins (the reference's
    truth-weighted formula, app/modules.py:476-482, with estimated instead of
    ideal assignments).  Built entirely from the existing HIP kernels:
    danet_separate_fwd -> argmax inside danet_attractor_truth_fwd.'''
    USE_TRUTH = False

    def __init__(self, model, name):
        super(KMeansEstimator, self).__init__(model, name)
        self.name = name

    def __call__(self, s_embed, s_src_pwr=None, s_mix_pwr=None, s_embed_flat=None):
        B, T, F, E = s_embed.shape
        C = hparams.MAX_N_SIGNAL
        v_anchors = self.model.get_variable(
            self.name + '/anchors', [hparams.NUM_ANCHOR, hparams.EMBED_SIZE],
            lambda shape, gen: torch.randn(shape, generator=gen, dtype=torch.float64).float())
        with torch.no_grad():
            s_embed_d = s_embed.detach()
            if s_mix_pwr is None:
                s_mix_pwr = torch.ones(B, T, F, device=s_embed.device)
            s_attr, _, _ = ops.AnchorAttractorFn.apply(s_embed_d, v_anchors.detach(), C)
            s_flat = s_embed_d.reshape(B, -1, E)
            for _ in range(int(hparams.KMEANS_ITERS)):
                # score[b,c,n] = |mix| * softmax_c(embed . attr): argmax_c = nearest attractor
                s_score, _ = ops.SeparateFn.apply(s_mix_pwr, s_attr, s_flat, 0, False)
                s_attr = ops.TruthAttractorFn.apply(
                    s_embed_d, s_score, s_mix_pwr, ops.TRUTH_MODES['truth-weighted'],
                    float(hparams.EPS))
        if hparams.DEBUG:
            self.debug_fetches = dict(anchors=v_anchors)
        return s_attr


@hparams.register_estimator('online')
class OnlineEstimator(Estimator):
    '''attractors updated frame by frame from the frames seen so far, after the Online Deep Attractor Network (Han,
    Wang, Luo, Mesgarani 2019) -- include/danet_online_hip.h.  NOT in the reference; an inference estimator with no
    backward.  The first T0 = ONLINE_INIT_FRAMES frames are the hold: the anchor estimator (the same `anchors` variable,
    name and shape, so the parameter files of `anchor` / `kmeans` load) gives A0 from them, and from frame T0 on every
    frame's attractors are the |mix|-weighted, soft-assigned means of the frames up to it, with the forgetting factor
    lambda = exp(-1 / ONLINE_MEMORY_FRAMES).  Returns the trajectory [B, T, C, E] (Model._separate sends it to
    ops.online_separate), or for a recording no longer than the hold the anchor estimator's [B, C, E], bit for bit.
    Causal in the embedding; the encoders are not causal, so this alone is not streaming.'''
    USE_TRUTH = False

    def __init__(self, model, name):
        super(OnlineEstimator, self).__init__(model, name)
        self.name = name

    def __call__(self, s_embed, s_src_pwr=None, s_mix_pwr=None, s_embed_flat=None):
        B, T, F, E = s_embed.shape
        C = hparams.MAX_N_SIGNAL
        T0, lam = self.model.online
        v_anchors = self.model.get_variable(
            self.name + '/anchors', [hparams.NUM_ANCHOR, hparams.EMBED_SIZE],
            lambda shape, gen: torch.randn(shape, generator=gen, dtype=torch.float64).float())
        s_a0, _, _ = ops.AnchorAttractorFn.apply(s_embed[:, :min(T0, T)].contiguous(), v_anchors, C)
        if hparams.DEBUG:
            self.debug_fetches = dict(anchors=v_anchors)
        if T <= T0:
            return s_a0                                      # [B, C, E]: the plain separator runs
        with torch.no_grad():
            if s_mix_pwr is None:
                s_mix_pwr = torch.ones(B, T, F, device=s_embed.device)
            s_traj = ops.online_attractors(s_embed.detach(), s_mix_pwr, s_a0.detach(), self.model.separator.ACT, lam, T0,
                                           float(hparams.EPS))
        if hparams.DEBUG:
            self.debug_fetches['attr_trajectory'] = s_traj
        return s_traj                                        # [B, T, C, E]


@hparams.register_estimator('truth-online')
class TruthOnlineEstimator(Estimator):
    '''the training twin of `online` (include/danet_tonline_hip.h): per-frame attractors that are the running,
    forgetting-weighted, |mix|-weighted means of the embedding under the IDEAL assignment of the frames seen so far, as
    the Online Deep Attractor Network is trained.  NOT in the reference.  Hold length and forgetting factor are those of
    the inference estimator (`model.online`: ONLINE_INIT_FRAMES, ONLINE_MEMORY_FRAMES), so it needs
    INFER_ESTIMATOR_METHOD = "online".  Always returns the trajectory [B, T, C, E], also for T <= T0; has an exact
    backward to the embedding and no parameters (the `anchors` of the hold's A0 are trained under "anchor" only).'''
    USE_TRUTH = True

    def __init__(self, model, name):
        super(TruthOnlineEstimator, self).__init__(model, name)

    def __call__(self, s_embed, s_src_pwr, s_mix_pwr, s_embed_flat=None):
        T0, lam = self.model.online
        s_traj = ops.TruthOnlineAttractorFn.apply(s_embed, s_src_pwr, s_mix_pwr, lam, T0, float(hparams.EPS))
        if hparams.DEBUG:
            self.debug_fetches = dict()
        return s_traj                                        # float[B, T, C, E]


class _DotSeparatorBase(Separator):
    ACT = None

    def __call__(self, s_mixed_signals_pwr, s_attractors, s_embed_flat):
        s_sep, s_masks = ops.SeparateFn.apply(
            s_mixed_signals_pwr, s_attractors, s_embed_flat, self.ACT, bool(hparams.DEBUG))
        if hparams.DEBUG:
            self.debug_fetches['masks'] = s_masks
        return s_sep                                         # [B, C, T, F]


@hparams.register_separator('dot-sigmoid-orig')
class DotSeparatorSigmoid(_DotSeparatorBase):
    '''sigmoid(embed . attractor) masks (app/modules.py:548-574)'''
    ACT = 1

    def __init__(self, model, name):
        super(DotSeparatorSigmoid, self).__init__(model, name)


@hparams.register_separator('dot-softmax-orig')
class DotSeparatorSoftmax(_DotSeparatorBase):
    '''softmax_c(embed . attractor) masks (app/modules.py:577-603)'''
    ACT = 0

    def __init__(self, model, name):
        super(DotSeparatorSoftmax, self).__init__(model, name)
