"""The strided rollout contract of include/ext/dstd_gcn_stride.h restated over
any window forward (tests/test_stride_host.py, tests/test_gpu_stride.py).

With Tin observed frames, T-frame windows, Tout = T - Tin, S = stride
(1 <= S <= Tout), H = horizon, K = ceil(H / S), m(s) = min(s, Tin - 1) and the
known sequence h = cat(obs, out) along the frame axis:

    x_k[:, s]        = h[:, k*S + m(s)]          s = 0..T-1
    y_k              = forward(x_k)
    out[:, k*S + j]  = y_k[:, Tin + j]           j = 0..S-1 while k*S + j < H

Window k needs h up to k*S + Tin - 1: what windows 0..k-1 have produced.  For
S = Tout this is ``predict_helper.predict_reference``, frame for frame.

``predict_strided_reference`` works on numpy arrays and on torch tensors alike
(the frame axis is 1; it only indexes and concatenates).  With a model as the
forward (``predict_strided_loop``) it is the loop a caller of ``model(x)``
writes today: the same kernels on windows built with torch indexing.
"""
import torch

from predict_helper import _cat


def predict_strided_reference(forward, obs, T, horizon, stride):
    """The ``horizon`` frames after ``obs`` [N, Tin, ...] under ``forward``
    ([N, T, ...] -> [N, T, ...]), ``stride`` frames kept per window."""
    Tin = obs.shape[1]
    assert 1 <= Tin < T and horizon >= 1 and 1 <= stride <= T - Tin
    m = [min(s, Tin - 1) for s in range(T)]
    h, have = obs, 0
    while have < horizon:
        x = h[:, [have + i for i in m]]
        y = forward(x)
        take = min(stride, horizon - have)
        h = _cat([h, y[:, Tin:Tin + take]])
        have += take
    return h[:, Tin:]


def predict_strided_loop(model, obs, horizon, stride):
    """``predict_strided_reference`` with the model's own eval forward, no autograd."""
    T = model.input_time_frame + model.output_time_frame
    with torch.no_grad():
        return predict_strided_reference(lambda x: model(x.contiguous()), obs, T, horizon, stride).contiguous()
