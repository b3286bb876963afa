"""Device-resident dataset and loader (include/dstd_gcn_data.h).

The reference feeds its engine from a ``torch.utils.data.DataLoader`` over four
float64 host arrays (``dataset/h36m.py:47-64``, ``cmu.py``, ``pw3d.py``): every
step casts and copies three of them to the GPU.  Those arrays are selections
of one -- frames and columns of ``all_seqs`` -- and its windows overlap T-fold.
``DeviceSequences`` keeps the distinct frames in device memory once, as
``float32(float64 value)`` (what the engine's per-batch ``.float()`` gives), and
``DeviceLoader`` yields the reference's 4-tuple ``(inputs, inputs_inv, targets,
all_seqs)`` as contiguous fp32 device tensors, one ``dstd_batch_gather`` launch
per batch: no DataLoader, no worker processes, no host-to-device copy and no
host synchronisation per step.  ``PredictionEngine.train`` / ``test`` take the
loader as they take the reference's.

A set may carry a group per window (an action of a test set: ``groups``,
``from_datasets``); ``PredictionEngine.test_groups`` then evaluates every group
in one pass over one loader (include/ext/dstd_gcn_eval.h).

``Augment`` describes continuous augmentations -- a per-sample rotation, scale
and shift of every joint, uniform noise on the observed frames -- that the
gather applies in its one launch (include/ext/dstd_gcn_augment.h):
``DeviceLoader(..., augment=Augment(...))``, or ``gather(index, transform=,
noise=, noise_seed=)`` for a caller's own transforms.  ``Augment(speed=)`` /
``gather(rate=)`` also play every window faster or slower, resampled in time in
that same launch from the frames a set built by ``from_sequences`` holds after
the window (include/ext/dstd_gcn_warp.h; ``room``, ``fit_rate``).

There is no CPU gather: a set built with ``device="cpu"`` serves the host-side
bookkeeping (weights, window starts, index order) only.
"""
import ctypes

import numpy as np
import torch

import dstd_native as native


def frame_maps(input_n, output_n, padding=True):
    """(i_idx, i_idx_inv) of the datasets (dataset/h36m.py:53-60): which window
    frame each frame of ``inputs`` / ``inputs_inv`` is.  With padding the
    output part repeats the last input frame (of the reversed window: frame
    output_n); without, the window itself and its reversal."""
    T = input_n + output_n
    if input_n < 1 or output_n < 0:
        raise ValueError(f"frame_maps: input_n {input_n}, output_n {output_n}")
    if padding:
        fwd = np.concatenate([np.arange(input_n), np.full(output_n, input_n - 1)])
        inv = np.concatenate([np.arange(output_n, T)[::-1], np.full(output_n, output_n)])
    else:
        fwd = np.arange(T)
        inv = fwd[::-1]
    return fwd.astype(np.int32), np.ascontiguousarray(inv).astype(np.int32)


def mirror_source(n_joints, left, right):
    """mirror_src of get_mirror (dataset/h36m.py:100-116) for the caller's
    joint lists: joint j of a mirrored window reads joint mirror_src[j]."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    if left.shape != right.shape or left.ndim != 1:
        raise ValueError("mirror: left and right joint lists of equal length")
    if len(left) and (min(left.min(), right.min()) < 0 or max(left.max(), right.max()) >= n_joints):
        raise ValueError(f"mirror: joint outside 0..{n_joints - 1}")
    ident = np.arange(n_joints)
    src = ident.copy()
    src[right] = ident[left]
    src[left] = ident[right]
    return src.astype(np.int32)


def mirror_frames(x, mirror_src):
    """x [..., D] float64 mirrored: joints exchanged, coordinate 0 negated."""
    m = x.reshape(*x.shape[:-1], -1, 3)[..., np.asarray(mirror_src, dtype=np.int64), :].copy()
    m[..., 0] = -m[..., 0]
    return m.reshape(x.shape)


def window_joint_weights(windows, dim_used):
    """(joint_weight_all, joint_weight_use) of dataset/h36m.py:93-98 over
    materialised windows [N][T][D], float64."""
    n, t, d = windows.shape
    x = windows.reshape(n, t, d // 3, 3)
    motion = np.mean(np.abs(x[:, 1:] - x[:, :-1]), (0, 1, 3))
    return _normalised_weights(motion, dim_used)


def _check_dim_used(dim_used, D):
    dim_used = np.asarray(dim_used, dtype=np.int64)
    if (dim_used.ndim != 1 or not 1 <= len(dim_used) <= D or dim_used[0] < 0 or dim_used[-1] >= D
            or np.any(np.diff(dim_used) <= 0)):
        raise ValueError("dim_used: strictly increasing columns of D")
    return dim_used


def _normalised_weights(motion, dim_used):
    with np.errstate(invalid="ignore", divide="ignore"):  # one joint, or none moving: NaN, as the reference
        w_all = (motion - motion.min()) / (motion.max() - motion.min())
    return w_all, w_all[np.unique(np.asarray(dim_used) // 3)]


class MeanStd:
    """The reference's MeanStdNorm interface (dataset/utils.py:2210-2236) for a
    (mean, std) pair over the used dims: numpy in, numpy out; tensor in,
    tensor out in the tensor's dtype and device (constants cached per both)."""

    def __init__(self, mean, std):
        self._mean = np.asarray(mean, dtype=np.float64).reshape(1, 1, -1)
        self._std = np.asarray(std, dtype=np.float64).reshape(1, 1, -1)
        self._cache = {}

    def _ms(self, data):
        if not isinstance(data, torch.Tensor):
            return self._mean, self._std
        key = (data.dtype, data.device)
        if key not in self._cache:
            # through fp32, as the reference's torch.Tensor(...) does
            self._cache[key] = tuple(torch.from_numpy(a).float().to(data.dtype).to(data.device)
                                     for a in (self._mean, self._std))
        return self._cache[key]

    def transform(self, data):
        m, s = self._ms(data)
        return (data - m) / s

    def inverse(self, data):
        m, s = self._ms(data)
        return data * s + m


def group_table(groups, n_windows, mirrored=False, group_names=None):
    """(table, names) of a grouped set: ``groups`` holds one non-negative int
    per stored window; the table has one int32 entry per window index, so with
    on-the-fly mirroring the half of the mirrored windows is appended (window
    w + N has the group of w).  ``names``: one string per group 0 ..
    max(groups), ``str(g)`` by default."""
    g = np.asarray(groups)
    if g.ndim != 1 or len(g) != n_windows or g.dtype.kind not in "iu":
        raise ValueError(f"groups: one int per stored window ({n_windows}), got {g.dtype} {g.shape}")
    if g.min() < 0 or g.max() >= 2 ** 31 - 1:
        raise ValueError("groups: non-negative ints")
    n_groups = int(g.max()) + 1
    if group_names is None:
        names = [str(k) for k in range(n_groups)]
    else:
        names = list(group_names)
        if len(names) != n_groups or not all(isinstance(n, str) for n in names) or len(set(names)) != n_groups:
            raise ValueError(f"group_names: {n_groups} distinct strings (one per group 0..{n_groups - 1}), "
                             f"got {names!r}")
    g = g.astype(np.int32)
    return (np.concatenate((g, g)) if mirrored else g), names


def _same_statistics(a, b):
    """Two scale transforms carry the same statistics (MeanStdNorm-like: _mean, _std)."""
    if a is b:
        return True
    if a is None or b is None:
        return False
    try:
        return all(np.array_equal(np.asarray(getattr(a, n)), np.asarray(getattr(b, n))) for n in ("_mean", "_std"))
    except AttributeError:
        return False


def _as_scaler(scaler):
    if scaler is None or (hasattr(scaler, "transform") and hasattr(scaler, "inverse")):
        return scaler
    mean, std = scaler
    return MeanStd(mean, std)


_FP32_MAX = float(np.finfo(np.float32).max)


def _check_augmentation(seqs, index, transform, noise, noise_seed):
    """The augmentation arguments of DeviceSequences.gather, checked before
    anything else (no device needed): (noise as a float, noise_seed mod 2^64)."""
    try:
        noise = float(noise)
    except (TypeError, ValueError):
        raise ValueError(f"noise: a non-negative finite amplitude, got {noise!r}") from None
    if not 0.0 <= noise <= _FP32_MAX:  # NaN fails both comparisons
        raise ValueError(f"noise: a non-negative finite (fp32) amplitude, got {noise!r}")
    if transform is not None:
        if seqs.scale_tsfm is not None or seqs._used is not None:
            raise ValueError("transform: a scaled set holds standardised coordinates, which a rigid transform "
                             "does not apply to (noise alone is allowed)")
        B = index.numel()
        if (not isinstance(transform, torch.Tensor) or transform.dtype != torch.float32
                or tuple(transform.shape) not in ((B, 12), (B, 3, 4)) or not transform.is_contiguous()
                or transform.device != seqs._frames.device):
            raise ValueError(f"transform: a contiguous float32 [{B}, 12] or [{B}, 3, 4] tensor on "
                             f"{seqs._frames.device}, got {_describe(transform)}")
    return noise, int(noise_seed) % 2 ** 64


def _check_rate(seqs, index, rate):
    """The ``rate`` argument of DeviceSequences.gather, checked before anything
    else (no device needed)."""
    if not isinstance(index, torch.Tensor):
        raise ValueError("index: a contiguous int64 vector on the set's device")
    B = index.numel()
    if (not isinstance(rate, torch.Tensor) or rate.dtype != torch.float32 or tuple(rate.shape) != (B,)
            or not rate.is_contiguous() or rate.device != seqs._frames.device):
        raise ValueError(f"rate: a contiguous float32 [{B}] tensor on {seqs._frames.device}, got {_describe(rate)}")


def _describe(t):
    if not isinstance(t, torch.Tensor):
        return type(t).__name__
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else ", not contiguous")


class Augment:
    """Continuous augmentations of a batch, applied inside the gather: a
    per-sample affine transform ``[A | t]`` of every joint, ``A = scale * R``,
    and a uniform jitter of the observed frames (``inputs`` / ``inputs_inv``).

    ``rotate``: ``(axis, max_angle)`` -- an angle uniform in ``[-max_angle,
    max_angle]`` (radians) about coordinate axis 0, 1 or 2; there is no
    default axis, the caller names the vertical of their data -- or ``"so3"``,
    a uniformly distributed rotation.  ``scale``: ``(lo, hi)``, uniform, ``0 <
    lo <= hi``.  ``shift``: an amplitude; each component of ``t`` is uniform in
    ``[-shift, shift]``.  ``noise``: the jitter's amplitude (not drawn here:
    the gather derives it from a seed, the window and the frame).

    ``speed``: ``(lo, hi)``, ``0 < lo <= hi`` -- a playback rate per sample,
    uniform in ``[lo, hi]``, at which the gather resamples the window in time
    (include/ext/dstd_gcn_warp.h).  Drawn by ``draw_speed``, from a generator
    of its own: ``draw`` does not know of it."""

    def __init__(self, rotate=None, scale=None, shift=None, noise=0.0, speed=None):
        if rotate is not None and rotate != "so3":
            try:
                axis, max_angle = rotate
                ok = axis in (0, 1, 2) and not isinstance(axis, bool) and 0.0 <= float(max_angle) < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f'rotate: (axis 0 / 1 / 2, max_angle >= 0) or "so3", got {rotate!r}')
            rotate = (int(axis), float(max_angle))
        if scale is not None:
            try:
                lo, hi = (float(v) for v in scale)
                ok = 0.0 < lo <= hi < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"scale: (lo, hi) with 0 < lo <= hi, got {scale!r}")
            scale = (lo, hi)
        if shift is not None:
            shift = float(shift)
            if not 0.0 <= shift < float("inf"):
                raise ValueError(f"shift: a non-negative finite amplitude, got {shift!r}")
        noise = float(noise)
        if not 0.0 <= noise <= _FP32_MAX:
            raise ValueError(f"noise: a non-negative finite (fp32) amplitude, got {noise!r}")
        if speed is not None:
            try:
                lo, hi = (float(v) for v in speed)
                ok = 0.0 < lo <= hi < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"speed: (lo, hi) with 0 < lo <= hi, got {speed!r}")
            speed = (lo, hi)
        self.rotate, self.scale, self.shift, self.noise, self.speed = rotate, scale, shift, noise, speed

    def draw_speed(self, B, generator, device):
        """One playback rate per sample: fp32 ``[B]`` on ``device``, uniform in
        ``[lo, hi]`` and clamped to it as ``scale`` is, or None without
        ``speed``.  One torch.rand on ``device`` fed from ``generator``; no host
        synchronisation."""
        if self.speed is None:
            return None
        lo, hi = self.speed
        u = torch.rand(B, generator=generator, device=torch.device(device), dtype=torch.float32)
        return (lo + (hi - lo) * u).clamp_(lo, hi)

    def draw(self, B, generator, device):
        """One ``[A | t]`` per sample: fp32 ``[B, 12]`` on ``device``, or None
        when neither rotate, scale nor shift is set.  Torch ops on ``device``
        fed from ``generator`` (a generator of that device), in the fixed
        order rotate, scale, shift; no host synchronisation."""
        if self.rotate is None and self.scale is None and self.shift is None:
            return None
        dev = torch.device(device)

        def rand(*shape):
            return torch.rand(*shape, generator=generator, device=dev, dtype=torch.float32)

        m = torch.zeros(B, 3, 4, dtype=torch.float32, device=dev)
        one = torch.ones(B, dtype=torch.float32, device=dev)
        if self.rotate == "so3":
            # a unit quaternion from four normals is uniform on the 3-sphere;
            # the homogeneous form of its matrix (|q|^2 on the diagonal, not 1)
            # stays orthogonal to first order when |q| is a few ulp off 1
            g = torch.randn(B, 4, generator=generator, device=dev, dtype=torch.float32)
            w, x, y, z = (g / g.norm(dim=1, keepdim=True).clamp_min(1e-30)).unbind(1)
            m[:, 0, 0] = (w * w + x * x) - (y * y + z * z)
            m[:, 1, 1] = (w * w + y * y) - (x * x + z * z)
            m[:, 2, 2] = (w * w + z * z) - (x * x + y * y)
            m[:, 0, 1], m[:, 1, 0] = 2 * (x * y - w * z), 2 * (x * y + w * z)
            m[:, 0, 2], m[:, 2, 0] = 2 * (x * z + w * y), 2 * (x * z - w * y)
            m[:, 1, 2], m[:, 2, 1] = 2 * (y * z - w * x), 2 * (y * z + w * x)
        elif self.rotate is not None:
            axis, max_angle = self.rotate
            i, j = (axis + 1) % 3, (axis + 2) % 3  # right-handed about `axis`
            theta = (2 * rand(B) - 1) * max_angle
            c, s = torch.cos(theta), torch.sin(theta)
            m[:, i, i], m[:, i, j], m[:, j, i], m[:, j, j] = c, -s, s, c
            m[:, axis, axis] = one  # the axis row and column: constants, never computed
        else:
            m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = one
        if self.scale is not None:
            lo, hi = self.scale
            k = (lo + (hi - lo) * rand(B)).clamp_(lo, hi)
            m[:, :, :3] *= k[:, None, None]  # 1 * k and 0 * k are exact
        if self.shift is not None:
            m[:, :, 3] = (2 * rand(B, 3) - 1) * self.shift
        return m.view(B, 12)


class DeviceSequences:
    """A dataset resident on the device: frames [F][D], windows as start rows.

    Build with ``from_windows``, ``from_sequences``, ``from_dataset`` or
    ``from_datasets``.  The reference dataset objects' attributes a runner
    reads are here: ``joint_weight_use`` / ``joint_weight_all``, ``dim_used``,
    ``time_tsfm`` (None), ``scale_tsfm``; plus ``nbytes`` (device memory held)
    and ``len`` (windows, the mirrored ones included).

    ``groups`` (one non-negative int per stored window; an action of a test
    set) makes the set a grouped one for ``PredictionEngine.test_groups``:
    ``groups`` is then the device int32 table with one entry per window index
    (a mirrored window w + N has the group of w), ``group_names`` one string
    per group (``str(g)`` by default) and ``n_groups`` their number.  Without
    it ``groups`` is None and the set counts as one group named "all"."""

    def __init__(self, frames, starts, seq_len, dim_used, input_n, output_n, padding, device, mirror_src=None,
                 scale_tsfm=None, joint_weights=None, groups=None, group_names=None, room=None):
        frames = np.asarray(frames, dtype=np.float64)
        starts = np.asarray(starts, dtype=np.int64)
        if frames.ndim != 2 or frames.shape[0] < 1 or frames.shape[1] % 3 != 0:
            raise ValueError(f"frames: expected [F][D] with D a multiple of 3, got {frames.shape}")
        F, D = frames.shape
        dim_used = _check_dim_used(dim_used, D)
        T = int(seq_len)
        if input_n + output_n != T or T < 1:
            raise ValueError(f"input_n {input_n} + output_n {output_n} is not the window length {T}")
        if starts.ndim != 1 or len(starts) < 1 or starts.min() < 0 or starts.max() + T > F:
            raise ValueError(f"starts: windows of {T} frames outside the {F} stored frames")
        if mirror_src is not None:
            mirror_src = np.asarray(mirror_src, dtype=np.int32)
            if mirror_src.shape != (D // 3,) or mirror_src.min() < 0 or mirror_src.max() >= D // 3:
                raise ValueError("mirror_src: one source joint per joint")
            if scale_tsfm is not None:
                raise ValueError("a scaled set stores its mirrored frames (no on-the-fly mirror)")
        self.device = torch.device(device)
        self.seq_len, self.input_n, self.output_n, self.padding = T, int(input_n), int(output_n), bool(padding)
        self.n_frames, self.n_dims, self.n_windows = F, D, len(starts)
        self.dim_used = dim_used
        self.time_tsfm = None
        self.scale_tsfm = scale_tsfm
        self.joint_weight_all, self.joint_weight_use = joint_weights if joint_weights is not None else (None, None)
        fwd, inv = frame_maps(input_n, output_n, padding)
        dev = self.device
        self._frames = torch.from_numpy(frames.astype(np.float32)).to(dev)
        self._used = None
        if scale_tsfm is not None:
            # (x - mean) / std in fp64 on the used columns, then the cast: what
            # the reference's arrays hold when the engine casts a batch
            used = np.asarray(scale_tsfm.transform(frames[None][:, :, dim_used]))[0]
            self._used = torch.from_numpy(np.ascontiguousarray(used).astype(np.float32)).to(dev)
        self._starts = torch.from_numpy(starts).to(dev)
        self._dim_used = torch.from_numpy(dim_used.astype(np.int32)).to(dev)
        self._frame_in, self._frame_inv = torch.from_numpy(fwd).to(dev), torch.from_numpy(inv).to(dev)
        self._mirror_src = torch.from_numpy(mirror_src).to(dev) if mirror_src is not None else None
        if groups is None:
            if group_names is not None:
                raise ValueError("group_names without groups")
            self.groups, self.group_names = None, ["all"]
        else:
            table, self.group_names = group_table(groups, self.n_windows, mirror_src is not None, group_names)
            self.groups = torch.from_numpy(table).to(dev)
        self.n_groups = len(self.group_names)
        self.room, self._room = None, None
        if room is not None:
            r = np.asarray(room)
            if r.ndim != 1 or len(r) != len(starts) or r.dtype.kind not in "iu":
                raise ValueError(f"room: one int per stored window ({len(starts)}), got {r.dtype} {r.shape}")
            r = r.astype(np.int64)
            if r.min() < T - 1 or (starts + r).max() > F - 1 or r.max() >= 2 ** 31:
                raise ValueError(f"room: {T - 1} <= room[n] and starts[n] + room[n] <= {F - 1} for every window")
            self.room = r.astype(np.int32)
            self._room = torch.from_numpy(self.room).to(dev)
        self._store = native.SeqStore(
            frames=self._frames.data_ptr(), used=self._used.data_ptr() if self._used is not None else None,
            starts=self._starts.data_ptr(), F=F, N=self.n_windows, T=T, D=D, Du=len(dim_used),
            dim_used=self._dim_used.data_ptr(), frame_in=self._frame_in.data_ptr(),
            frame_inv=self._frame_inv.data_ptr(),
            mirror_src=self._mirror_src.data_ptr() if self._mirror_src is not None else None)

    # ---- constructors ---------------------------------------------------------------
    @classmethod
    def from_windows(cls, all_seqs, dim_used, input_n, output_n, padding=True, device="cuda", mirror=None,
                     scaler=None, groups=None, group_names=None):
        """Materialised windows [N][T][D] (what load_data_3d returns), stored
        back to back.  mirror=(left, right) joint lists doubles the set as
        get_mirror does; scaler: a MeanStdNorm-like object, (mean, std), or
        True for the statistics of the used columns over every window frame
        (dataset/h36m.py:81-85).  groups: one int per window of all_seqs (a
        mirrored window inherits its group)."""
        w = np.asarray(all_seqs, dtype=np.float64)
        if w.ndim != 3 or w.shape[2] % 3 != 0 or w.shape[1] < 2:
            raise ValueError(f"all_seqs: expected [N][T >= 2][D], D a multiple of 3, got {w.shape}")
        dim_used = _check_dim_used(dim_used, w.shape[2])
        mirror_src = mirror_source(w.shape[2] // 3, *mirror) if mirror is not None else None
        full = w if mirror_src is None else np.concatenate((w, mirror_frames(w, mirror_src)), axis=0)
        weights = window_joint_weights(full, dim_used)
        if groups is not None and len(np.asarray(groups)) != w.shape[0]:
            raise ValueError(f"groups: one int per window ({w.shape[0]}), got {len(np.asarray(groups))}")
        if scaler is not None:  # mirror, then statistics, then scale -- on stored mirrored frames
            if groups is not None and mirror_src is not None:
                groups = np.concatenate((np.asarray(groups), np.asarray(groups)))
            w, mirror_src = full, None
            if scaler is True:
                u = w[:, :, np.asarray(dim_used)].reshape(w.shape[0] * w.shape[1], -1)
                scaler = (np.mean(u, axis=0), np.std(u, axis=0))
        n, t, d = w.shape
        return cls(w.reshape(n * t, d), np.arange(n, dtype=np.int64) * t, t, dim_used, input_n, output_n, padding,
                   device, mirror_src, _as_scaler(scaler), weights, groups, group_names)

    @classmethod
    def from_sequences(cls, sequences, seq_len, dim_used, input_n, output_n, padding=True, device="cuda",
                       mirror=None, scaler=None, groups=None, group_names=None):
        """Whole sequences [F_i][D]: every start 0..F_i - seq_len of every
        sequence is a window (the training selection of load_data_3d,
        dataset/utils.py:860-866), frames stored once.  The joint weights come
        from how many windows hold each pair of consecutive frames.  groups:
        one int per sequence, which every window of the sequence inherits."""
        seqs = [np.asarray(s, dtype=np.float64) for s in sequences]
        T = int(seq_len)
        if not seqs or any(s.ndim != 2 or s.shape[1] != seqs[0].shape[1] or s.shape[0] < T for s in seqs) or T < 2:
            raise ValueError(f"sequences: [F_i][D] arrays of at least seq_len = {T} >= 2 frames each")
        D = seqs[0].shape[1]
        if D % 3 != 0:
            raise ValueError(f"sequences: D = {D} is not a multiple of 3")
        dim_used = _check_dim_used(dim_used, D)
        mirror_src = mirror_source(D // 3, *mirror) if mirror is not None else None
        if scaler is True:
            raise ValueError("from_sequences takes the scaler's statistics from the caller")
        if groups is not None:
            groups = np.asarray(groups)
            if groups.ndim != 1 or len(groups) != len(seqs):
                raise ValueError(f"groups: one int per sequence ({len(seqs)}), got shape {groups.shape}")
        if scaler is not None and mirror_src is not None:
            seqs = seqs + [mirror_frames(s, mirror_src) for s in seqs]
            groups = np.concatenate((groups, groups)) if groups is not None else None
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
        starts = np.concatenate([off + np.arange(len(s) - T + 1) for off, s in zip(offsets, seqs)])
        # a window's room: the frames of its own sequence from its start on (what a faster playback may read)
        room = np.concatenate([len(s) - 1 - np.arange(len(s) - T + 1) for s in seqs])
        if groups is not None:
            groups = np.repeat(groups, [len(s) - T + 1 for s in seqs])
        # mean |x[t+1] - x[t]| over every window: pair p of a sequence lies in
        # windows max(0, p - T + 2) .. min(p, F_i - T)
        motion = np.zeros(D // 3)
        for s in seqs:
            p = np.arange(len(s) - 1)
            mult = np.minimum(p, len(s) - T) - np.maximum(0, p - T + 2) + 1
            motion += (np.abs(np.diff(s, axis=0)).reshape(len(p), -1, 3).sum(2) * mult[:, None]).sum(0)
        if mirror_src is not None and scaler is None:  # the mirrored half moves joint j as mirror_src[j] moves
            motion = (motion + motion[mirror_src]) / 2
        motion /= len(starts) * (T - 1) * 3
        if scaler is not None:
            mirror_src = None
        return cls(np.concatenate(seqs, axis=0), starts, T, dim_used, input_n, output_n, padding, device, mirror_src,
                   _as_scaler(scaler), _normalised_weights(motion, dim_used), groups, group_names, room=room)

    @classmethod
    def from_dataset(cls, ds, input_n, output_n, padding=True, device="cuda"):
        """A reference dataset object (Human36M, CMUMocap, PW3D) as it is: its
        all_seqs (mirrored windows already appended), dim_used, scale_tsfm and
        joint weights."""
        w = np.asarray(ds.all_seqs, dtype=np.float64)
        n, t, d = w.shape
        return cls(w.reshape(n * t, d), np.arange(n, dtype=np.int64) * t, t, ds.dim_used, input_n, output_n, padding,
                   device, None, getattr(ds, "scale_tsfm", None), (ds.joint_weight_all, ds.joint_weight_use))

    @classmethod
    def from_datasets(cls, datasets, input_n, output_n, padding=True, device="cuda"):
        """An ordered mapping {name: reference dataset object} (the runners'
        per-action test sets, one Human36M / CMUMocap per action) as one
        grouped set: their all_seqs back to back in mapping order, one group
        per entry.  dim_used, window length and D must agree; the scale_tsfm
        is the first entry's, and the others must carry the same statistics.
        A test set: no joint weights."""
        items = list(datasets.items())
        if not items:
            raise ValueError("from_datasets: no dataset")
        names = [str(k) for k, _ in items]
        first = items[0][1]
        dim_used = np.asarray(first.dim_used)
        scale = getattr(first, "scale_tsfm", None)
        windows, groups = [], []
        for g, (name, ds) in enumerate(items):
            w = np.asarray(ds.all_seqs, dtype=np.float64)
            if w.ndim != 3 or (windows and w.shape[1:] != windows[0].shape[1:]):
                raise ValueError(f"from_datasets: all_seqs of '{name}' is {w.shape}, "
                                 f"'{names[0]}' has windows of {windows[0].shape[1:] if windows else '[T][D]'}")
            if not np.array_equal(np.asarray(ds.dim_used), dim_used):
                raise ValueError(f"from_datasets: dim_used of '{name}' differs from that of '{names[0]}'")
            if not _same_statistics(scale, getattr(ds, "scale_tsfm", None)):
                raise ValueError(f"from_datasets: scale_tsfm of '{name}' differs from that of '{names[0]}'")
            windows.append(w)
            groups.append(np.full(len(w), g, dtype=np.int64))
        w = np.concatenate(windows, axis=0)
        n, t, d = w.shape
        return cls(w.reshape(n * t, d), np.arange(n, dtype=np.int64) * t, t, dim_used, input_n, output_n, padding,
                   device, None, scale, None, np.concatenate(groups), names)

    # ---- the set --------------------------------------------------------------------
    def __len__(self):
        return self.n_windows * (2 if self._mirror_src is not None else 1)

    @property
    def nbytes(self):
        """Device memory the set holds."""
        held = (self._frames, self._used, self._starts, self._dim_used, self._frame_in, self._frame_inv,
                self._mirror_src, self.groups, self._room)
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    @property
    def starts(self):
        return self._starts

    def fit_rate(self, index, rate):
        """``rate`` (fp32 [B] on the set's device) capped per sample so that
        the last frame of the warped window still lies in the window's room:
        ``min(rate, room[w] / (T - 1))``, w the index folded over the mirrored
        half; the cap is 1 on a set without a room table.  Indices outside the
        set keep their rate (the gather skips those rows).  Torch ops on the
        device, no host synchronisation.  The gather itself never reads past
        the room -- a position beyond it shows the last frame in room -- so
        this is what keeps an augmented window from freezing at the end of its
        recording, not what keeps the reads in bounds."""
        n = self.n_windows
        w = torch.where(index >= n, index - n, index) if self._mirror_src is not None else index
        ok = (w >= 0) & (w < n)
        if self._room is None:
            return torch.where(ok, rate.clamp(max=1.0), rate)
        # the quotient rounded DOWN to fp32 (fp64 holds it to well below an fp32 ulp), so that
        # cap * (T - 1) <= room exactly and the kernel's fp32 product cannot round past the room
        exact = self._room[w.clamp(0, n - 1)].to(torch.float64) / float(max(self.seq_len - 1, 1))
        cap = exact.to(torch.float32)
        cap = torch.where(cap.to(torch.float64) > exact, torch.nextafter(cap, torch.zeros_like(cap)), cap)
        return torch.where(ok, torch.minimum(rate, cap), rate)

    def gather(self, index, outputs=("inputs", "inputs_inv", "targets", "all_seqs"), out=None, transform=None,
               noise=0.0, noise_seed=0, rate=None):
        """(inputs, inputs_inv, targets, all_seqs) of the windows ``index``
        (int64 device tensor [B]) by one dstd_batch_gather on the current
        stream; a name missing from ``outputs`` is not produced (None).
        ``out``: tensors to write into instead of fresh ones, by name.

        ``transform`` (contiguous fp32 [B, 12] or [B, 3, 4] on the set's
        device: a row-major 3x4 [A | t] per sample, applied to every joint of
        all four tensors) and ``noise`` (amplitude of a uniform jitter of
        ``inputs`` / ``inputs_inv`` alone, keyed by ``noise_seed``, the window
        and the source frame) augment the batch in the same single launch
        (dstd_batch_gather_aug, include/ext/dstd_gcn_augment.h).  A scaled set
        takes noise, in the scaler's units, but no transform.

        ``rate`` (contiguous fp32 [B] on the set's device: a playback speed per
        sample) resamples every window in time, again in the same launch
        (dstd_batch_gather_warp, include/ext/dstd_gcn_warp.h): window frame f
        shows the recording at f * rate frames past the window's start,
        blended linearly from the two stored frames around it, and all four
        tensors are views of that warped window.  A window reads no further
        than its room (``room``; ``fit_rate`` caps a rate to it).  A scaled
        set takes a rate."""
        if rate is not None:
            _check_rate(self, index, rate)
        noise, noise_seed = _check_augmentation(self, index, transform, noise, noise_seed)
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceSequences.gather runs on the MI355X only (the set is on {self.device}); "
                               "there is no CPU fallback")
        if index.dtype != torch.int64 or index.device != self._frames.device or index.dim() != 1 \
                or not index.is_contiguous():
            raise ValueError("index: a contiguous int64 vector on the set's device")
        B = index.numel()
        shapes = {n: (B, self.seq_len, self.n_dims if n == "all_seqs" else len(self.dim_used))
                  for n in ("inputs", "inputs_inv", "targets", "all_seqs")}
        res = {}
        for n in outputs:
            t = out[n] if out is not None and n in out else torch.empty(shapes[n], dtype=torch.float32,
                                                                        device=self._frames.device)
            if tuple(t.shape) != shapes[n]:
                raise ValueError(f"{n}: expected {shapes[n]}, got {tuple(t.shape)}")
            res[n] = t
        p = {n: native.ptr(t, n) for n, t in res.items()}
        if rate is not None:
            code = native.lib().dstd_batch_gather_warp(
                native.ext_warp.seq_store_ref(self._store), self._room.data_ptr() if self._room is not None else None,
                index.data_ptr(), B, rate.data_ptr(), transform.data_ptr() if transform is not None else None, noise,
                noise_seed, p.get("inputs"), p.get("inputs_inv"), p.get("targets"), p.get("all_seqs"),
                native.stream_handle(self._frames.device))
            native.check(code, "dstd_batch_gather_warp")
        elif transform is None and noise == 0.0:
            code = native.lib().dstd_batch_gather(ctypes.byref(self._store), index.data_ptr(), B, p.get("inputs"),
                                                  p.get("inputs_inv"), p.get("targets"), p.get("all_seqs"),
                                                  native.stream_handle(self._frames.device))
            native.check(code, "dstd_batch_gather")
        else:
            code = native.lib().dstd_batch_gather_aug(
                native.ext_augment.seq_store_ref(self._store), index.data_ptr(), B,
                transform.data_ptr() if transform is not None else None, noise, noise_seed, p.get("inputs"),
                p.get("inputs_inv"), p.get("targets"), p.get("all_seqs"), native.stream_handle(self._frames.device))
            native.check(code, "dstd_batch_gather_aug")
        return tuple(res.get(n) for n in ("inputs", "inputs_inv", "targets", "all_seqs"))


class DeviceLoader:
    """Batches of a DeviceSequences in the reference loader's shape: iterating
    yields ``(inputs, inputs_inv, targets, all_seqs)``, fp32 on the device,
    one launch per batch and no host synchronisation.  Indices are generated
    on the set's device; ``shuffle`` draws a permutation per epoch from a
    device generator seeded ``seed + epoch`` (epochs counted per iteration
    started).  ``last_index`` is the index tensor of the batch just yielded.

    ``augment`` (an ``Augment``) transforms and jitters every batch inside its
    gather.  The transforms come from a generator of their own, seeded ``seed
    + epoch`` when an epoch starts, so the order of windows is the same with
    and without augmentation; batch ``i`` of an epoch uses the noise seed
    ``noise_seed(seed, epoch, i)``.  ``last_transform`` and ``last_noise_seed``
    describe the batch just yielded (None without ``augment``).

    With ``Augment(speed=...)`` every batch is also resampled in time: the
    rates come from a third generator of their own, seeded ``rate_seed(seed,
    epoch)`` when an epoch starts -- ``seed + epoch`` under a fixed tag, so that
    its stream is not the transform generator's: from the same seed a rate and
    a rotation angle would be drawn from the same uniform -- once per batch,
    and capped by the set's ``fit_rate``.  The order of windows, the transforms
    and the noise seeds are the same with and without ``speed``.  ``last_rate``
    is the capped rate tensor of the batch just yielded (None without
    ``speed``)."""

    def __init__(self, seqs, batch_size, shuffle=False, drop_last=False, seed=0, augment=None):
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.seqs, self.batch_size = seqs, int(batch_size)
        self.shuffle, self.drop_last, self.seed = bool(shuffle), bool(drop_last), int(seed)
        self.epoch = 0
        self.last_index = None
        self._order = None
        self._generator = None
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError(f"augment: an Augment or None, got {type(augment).__name__}")
        self.augment = augment
        self.last_transform = self.last_noise_seed = self.last_rate = None
        self._aug_generator = self._rate_generator = None

    def __len__(self):
        n = len(self.seqs)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def index_batches(self):
        """The epoch's index tensors, one per batch (what ``__iter__`` gathers)."""
        n, dev = len(self.seqs), self.seqs.device
        if self.shuffle:
            if self._generator is None:
                self._generator = torch.Generator(device=dev)
            self._generator.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=self._generator, device=dev)
        else:
            if self._order is None:
                self._order = torch.arange(n, dtype=torch.int64, device=dev)
            order = self._order
        self.epoch += 1
        for i in range(len(self)):
            yield order[i * self.batch_size:(i + 1) * self.batch_size]

    @staticmethod
    def noise_seed(seed, epoch, i):
        """The noise seed of batch ``i`` of epoch ``epoch`` (Python ints)."""
        return (((int(seed) + int(epoch)) << 32) ^ int(i)) % 2 ** 64

    RATE_STREAM = 0x9E3779B97F4A7C15  # tag of the rate generator's seed

    @classmethod
    def rate_seed(cls, seed, epoch):
        """The seed of the rate generator of epoch ``epoch`` (Python ints):
        ``seed + epoch`` with a fixed tag xor-ed in.  The transform generator is
        seeded ``seed + epoch`` itself and its first draw can be one
        ``rand(B)``, as a rate draw is: from the same seed every sample's rate
        would be a function of its rotation angle."""
        return ((int(seed) + int(epoch)) ^ cls.RATE_STREAM) % 2 ** 64

    def __iter__(self):
        aug = self.augment
        if aug is None:
            for idx in self.index_batches():
                self.last_index = idx
                yield self.seqs.gather(idx)
            return
        epoch, dev = self.epoch, self.seqs.device  # index_batches counts the epoch when its first batch is drawn
        if self._aug_generator is None:
            self._aug_generator = torch.Generator(device=dev)
        self._aug_generator.manual_seed(self.seed + epoch)
        if aug.speed is not None:
            if self._rate_generator is None:
                self._rate_generator = torch.Generator(device=dev)
            self._rate_generator.manual_seed(self.rate_seed(self.seed, epoch))
        for i, idx in enumerate(self.index_batches()):
            self.last_index = idx
            self.last_transform = aug.draw(idx.numel(), self._aug_generator, dev)
            self.last_noise_seed = self.noise_seed(self.seed, epoch, i)
            self.last_rate = None
            if aug.speed is not None:
                self.last_rate = self.seqs.fit_rate(idx, aug.draw_speed(idx.numel(), self._rate_generator, dev))
            yield self.seqs.gather(idx, transform=self.last_transform, noise=aug.noise,
                                   noise_seed=self.last_noise_seed, rate=self.last_rate)


__all__ = ["Augment", "DeviceSequences", "DeviceLoader", "MeanStd", "frame_maps", "group_table", "mirror_source"]
