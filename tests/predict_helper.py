"""The rollout contract of include/dstd_gcn_predict.h restated over any window
forward (tests/test_predict_host.py, tests/test_gpu_predict.py).

With Tin observed frames, T-frame windows, Tout = T - Tin and m(s) = min(s, Tin - 1):

    x_0[:, s]     = obs[:, m(s)]
    y_k           = forward(x_k)
    seq_k         = cat(x_k[:, :Tin], y_k[:, Tin:])
    out           = cat_k y_k[:, Tin:], cut to `horizon` frames
    x_{k+1}[:, s] = seq_k[:, T - Tin + m(s)]

``predict_reference`` works on numpy arrays and on torch tensors alike (the
frame axis is 1; it only indexes and concatenates), so the same loop is the
fp64 restatement of the host tests and, with a model as the forward
(``predict_loop``), what a caller of ``model(x)`` writes today: the same
kernels on windows built with torch indexing.
"""
import numpy as np
import torch


def _cat(parts):
    return torch.cat(parts, 1) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts, 1)


def predict_reference(forward, obs, T, horizon):
    """The ``horizon`` frames after ``obs`` [N, Tin, ...] under ``forward``
    ([N, T, ...] -> [N, T, ...])."""
    Tin = obs.shape[1]
    assert 1 <= Tin < T and horizon >= 1
    m = [min(s, Tin - 1) for s in range(T)]
    x = obs[:, m]
    outs, have = [], 0
    while have < horizon:
        y = forward(x)
        take = min(T - Tin, horizon - have)
        outs.append(y[:, Tin:Tin + take])
        have += take
        seq = _cat([x[:, :Tin], y[:, Tin:]])
        x = seq[:, [T - Tin + i for i in m]]
    return _cat(outs)


def predict_loop(model, obs, horizon):
    """``predict_reference`` with the model's own eval forward, no autograd."""
    T = model.input_time_frame + model.output_time_frame
    with torch.no_grad():
        return predict_reference(lambda x: model(x.contiguous()), obs, T, horizon).contiguous()
