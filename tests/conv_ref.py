'''
Float64 torch-CPU restatement of the reference's `conv-bilstm-v1` encoder (app/modules.py:263-379)
and of a whole model step around it -- the authority the GPU tests of the conv encoder compare with
(tests/test_gpu_conv.py, tests/test_gpu_conv_encoder.py).  Test infrastructure only.

Convolutions are torch.nn.functional's, weights in TF's [k, k, Cin, Cout] order; leaky ReLU is
F.leaky_relu, whose gradient at exactly 0 is alpha like tf.maximum(alpha * z, z); max-pool is
F.max_pool2d (gradient to the first maximum of a window, row-major).
'''
import torch
import torch.nn.functional as Fn

from oracle import torch_ref as R


def conv(x, w, b, alpha, pool=False):
    '''tf.layers.conv2d(channels_first, 'same', leaky-ReLU activation) [+ 2x2 / 2 'valid' max-pool]'''
    k = w.shape[0]
    z = Fn.conv2d(x, w.permute(3, 2, 0, 1), b, padding=k // 2)
    y = Fn.leaky_relu(z, alpha)
    return Fn.max_pool2d(y, 2, 2) if pool else y


def depth_to_space(x):
    '''modules.py:350-358, block 2: [B, C, T, F] -> [B, C/4, 2T, 2F] with
    out[c][2t+a][2f+b] = x[4c+2a+b][t][f] (the encoder: [B, 64, T/4, nfft/8] -> [B, 16, T/2, nfft/4])'''
    B, C, T, F = x.shape
    x = x.reshape(B, C // 4, 2, 2, T, F).permute(0, 1, 4, 2, 5, 3)
    return x.reshape(B, C // 4, 2 * T, 2 * F)


def _center(x):
    return x - x.mean(dim=(1, 2, 3), keepdim=True)


def encoder(x, params, nfft, E, alpha, fetches=None):
    '''x [B, T, F] -> embed [B, T, F, E]; params keyed by TF variable name'''
    def p(n):
        return params['global/encoder/' + n]

    def c(h, i, pool=False):
        n = 'conv2d' if i == 0 else 'conv2d_%d' % i
        return conv(h, p(n + '/kernel'), p(n + '/bias'), alpha, pool)

    B, T, F = x.shape
    h = c(x[:, None], 0)
    h = c(h, 1, pool=True)
    h = c(h, 2)
    h = c(h, 3, pool=True)
    s_mid1 = _center(h)                                                  # [B, 16, T/4, nfft/8]
    s = s_mid1.transpose(1, 2).reshape(B, -1, 2 * nfft)
    for l in range(2):
        fwd = R.lstm_scan(s, p('lstm%d_fwd/LSTM/linear/W' % l), p('lstm%d_fwd/LSTM/linear/B' % l), nfft)
        bwd = R.lstm_scan(s, p('lstm%d_bwd/LSTM/linear/W' % l), p('lstm%d_bwd/LSTM/linear/B' % l), nfft,
                          reverse=True)
        s = torch.cat([fwd, bwd], dim=-1)
    s_mid3 = s.reshape(B, -1, 16, nfft // 8).transpose(1, 2)
    s_mid3 = _center(s_mid3 + s_mid1)
    h = c(s_mid3, 4)
    mid4 = depth_to_space(c(h, 5))
    h = c(mid4, 6)
    h = c(h, 7)                                                          # [B, 8, T/2, nfft/4]
    rows = h.transpose(1, 2).reshape(B, -1, nfft)
    out = rows @ p('dense/kernel')
    if fetches is not None:
        fetches.update(conv_act=s_mid1, lstm_act=s_mid3, mid4=mid4)
    return out.reshape(B, T, F, E)


def model_forward(src, params, cfg):
    '''main.py:208-309 (train branch) with this encoder; cfg: nfft, E, C, alpha, train_est, separator'''
    fe = R.frontend(src)
    E, C, eps = cfg['E'], cfg['C'], cfg.get('eps', 1e-7)
    embed = encoder(fe['mix_log'], params, cfg['nfft'], E, cfg['alpha'])
    B = embed.shape[0]
    ef = embed.reshape(B, -1, E)
    if cfg['train_est'] == 'anchor':
        attrs = R.est_anchor(embed, params['global/train_estimator/anchors'], C)
    else:
        fn = {'truth': R.est_truth, 'truth-threshold': R.est_truth_threshold,
              'truth-weighted': R.est_truth_weighted}[cfg['train_est']]
        attrs = fn(embed, fe['src_pwr'], fe['mix_pwr'], eps)
    act = {'dot-softmax-orig': 'softmax', 'dot-sigmoid-orig': 'sigmoid'}[cfg['separator']]
    sep_pwr, _ = R.sep_dot(fe['mix_pwr'], attrs, ef, act)
    ph = fe['phase'][:, None]
    sep = torch.complex(torch.cos(ph) * sep_pwr, torch.sin(ph) * sep_pwr)
    loss, perms, idx = R.pit_mse_loss(src, sep)
    sep_perm = sep[torch.arange(B)[:, None], perms[idx]]
    snr = R.batch_snr(src, sep_perm, eps).mean()
    return dict(embed=embed, loss=loss, SNR=snr)
