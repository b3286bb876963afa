"""Refusal codes of the training entry points (include/dstd_gcn_train.h), on
the host: a refused call returns before any HIP work, so no GPU is needed.

Every call here is refused.  Device pointers are the dummy address PTR and are
never dereferenced.  Per entry point the BASE row passes every check except a
saved_bytes one short of the export (-2), which shows that the rows below it --
the base with one thing changed -- fail at the check they name and not at an
earlier one.  The order of the checks is part of what is pinned: pointers /
flags / PAIRED parity (-1), non-positive shape (-1), envelope (-3), sizes (-2).
"""
import ctypes
import re

import pytest

from conftest import ROOT  # noqa: F401  (puts the package on sys.path)
import dstd_native as native

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3
PTR = 0x1000
SHORT, FULL = "export - 1", "export"
MODEL_L = 1  # layers of the model rows: enc[0] is populated, enc[1:] stay NULL


def _noop_collective(*a):
    return 0


_FN = native.COLLECTIVE_FN(_noop_collective)
_NULL_FN = native.COLLECTIVE_FN()


def fill(s):
    """Every pointer member of a ctypes structure (nested ones included) = PTR."""
    for name, typ in s._fields_:
        if typ is ctypes.c_void_p:
            setattr(s, name, PTR)
        elif typ is ctypes.c_float:
            setattr(s, name, 1e-5)
        elif issubclass(typ, ctypes.Structure):
            fill(getattr(s, name))
        elif issubclass(typ, ctypes.Array):
            arr = getattr(s, name)
            for i in range(len(arr)):
                if typ._type_ is ctypes.c_void_p:
                    arr[i] = PTR
                else:
                    fill(arr[i])
    return s


def leaves(s, prefix):
    """Paths ('p.conv_s.1.wf') of every pointer member of a structure."""
    for name, typ in s._fields_:
        path = f"{prefix}.{name}"
        if typ is ctypes.c_void_p:
            yield path
        elif isinstance(typ, type) and issubclass(typ, ctypes.Structure):
            yield from leaves(getattr(s, name), path)
        elif isinstance(typ, type) and issubclass(typ, ctypes.Array):
            arr = getattr(s, name)
            for i in range(len(arr)):
                if typ._type_ is ctypes.c_void_p:
                    yield f"{path}.{i}"
                else:
                    yield from leaves(arr[i], f"{path}.{i}")


def _walk(args, path):
    parts = path.split(".")
    obj = args[parts[0]]
    for k in parts[1:-1]:
        obj = obj[int(k)] if k.isdigit() else getattr(obj, k)
    return obj, parts[-1]


def get_path(args, path):
    if "." not in path:
        return args[path]
    obj, last = _walk(args, path)
    v = obj[int(last)] if last.isdigit() else getattr(obj, last)
    return ctypes.cast(v, ctypes.c_void_p).value if isinstance(v, native.COLLECTIVE_FN) else v


def set_path(args, path, value):
    if "." not in path:
        args[path] = value
        return
    obj, last = _walk(args, path)
    if last.isdigit():
        obj[int(last)] = value
    else:
        setattr(obj, last, value)


def differs(a, base, path):
    if path.split(".")[0] != path and base[path.split(".")[0]] is None:
        return True  # a member of a structure the base row does not pass
    return get_path(a, path) != get_path(base, path)


def clone(args):
    return {k: type(v).from_buffer_copy(v) if isinstance(v, ctypes.Structure) else v for k, v in args.items()}


def block_params(cin, cout):
    p = fill(native.BlockParams())
    p.cin, p.cout = cin, cout
    return p


def model_params(T, V, C, L):
    p = native.ModelParams()
    p.T, p.V, p.num_layers, p.num_feature, p.in_channels = T, V, L, C, 6
    for blk, (ci, co) in ((p.st_in, (6, C)), (p.st_out, (C, 3))):
        fill(blk)
        blk.cin, blk.cout = ci, co
    fill(p.bn_in)
    p.prelu = PTR
    for i in range(L):
        fill(p.enc[i])
        p.enc[i].cin = p.enc[i].cout = C
        fill(p.enc_bn[i])
        p.enc_prelu[i] = PTR
    return p


def model_grads(L):
    g = native.ModelGrads()
    fill(g.st_in), fill(g.st_out), fill(g.bn_in)
    g.prelu = PTR
    for i in range(L):
        fill(g.enc[i]), fill(g.enc_bn[i])
        g.enc_prelu[i] = PTR
    return g


def bn_sync(world=2, rank=0, C=64, V=3):
    return native.BnSyncStruct(world, rank, _FN, None, PTR, int(native.lib().dstd_bn_sync_buffer_floats(world, C, V)))


def beyond_layers(path):
    m = re.match(r"[pg]\.(enc|enc_bn|enc_prelu)\.(\d+)", path)
    return bool(m) and int(m.group(2)) >= MODEL_L


# ---------------------------------------------------------------------------
# the six entry points: argument order, base row, size exports
# ---------------------------------------------------------------------------
class Entry:
    def __init__(self, fn, order, base, sizes, accepted=()):
        self.fn, self.order, self.base, self.sizes, self.accepted = fn, order, base, sizes, set(accepted)

    def exports(self, a):
        """{size argument: its export at the shape of row a}."""
        L = native.lib()
        return {k: int(getattr(L, f)(*dims(a))) for k, (f, dims) in self.sizes.items()}

    def resolve(self, a, shape_of):
        """SHORT / FULL size arguments -> bytes, from the exports at shape_of's shape."""
        ex = self.exports(shape_of)
        out = dict(a)
        for k in self.sizes:
            if a[k] == SHORT:
                out[k] = ex[k] - 1
            elif a[k] == FULL:
                out[k] = ex[k]
        return out

    def call(self, a):
        argv = [ctypes.byref(a[k]) if isinstance(a[k], ctypes.Structure) else a[k] for k in self.order]
        return getattr(native.lib(), self.fn)(*argv)


def _op_dims(a):
    return (a["mode"], a["B"], a["cin"], a["cout"], a["T"], a["V"], a["red"])


def _blk_dims(a):
    return (a["B"], a["p"].cin, a["p"].cout, a["T"], a["V"])


def _mdl_dims(a):
    p = a["p"]
    return (a["B"], p.T, p.V, p.num_feature, p.num_layers)


OP_SHAPE = dict(mode=0, B=2, cin=5, cout=7, T=4, V=3, red=2)
OP_SIZES = {"saved_bytes": ("dstd_dstdgc_train_saved_bytes_r", _op_dims),
            "workspace_bytes": ("dstd_dstdgc_train_workspace_bytes_r", _op_dims)}
BLK_SIZES = {"saved_bytes": ("dstd_block_train_saved_bytes", _blk_dims),
             "workspace_bytes": ("dstd_block_train_workspace_bytes", _blk_dims)}
MDL_SIZES = {"saved_bytes": ("dstd_model_train_saved_bytes", _mdl_dims),
             "workspace_bytes": ("dstd_model_train_workspace_bytes", _mdl_dims)}
# residual members are not read (nor checked) when cin == cout: the model's encoder
ENC_RES = [f"{s}.enc.0.{m}" for s, ms in (("p", ("res_w", "res_b", "res_bn.weight", "res_bn.bias",
                                                  "res_bn.running_mean", "res_bn.running_var")),
                                          ("g", ("res_w", "res_b", "res_bn.weight", "res_bn.bias"))) for m in ms]


def entries():
    fwd_only = lambda sizes: {k: v for k, v in sizes.items() if k == "saved_bytes"}  # noqa: E731
    return {
        "op_fwd": Entry(
            "dstd_dstdgc_train_fwd_r",
            "mode x B cin cout T V red w A alpha y saved saved_bytes stream".split(),
            dict(OP_SHAPE, x=PTR, w=fill(native.GCWeights()), A=PTR, alpha=PTR, y=PTR, saved=PTR, saved_bytes=SHORT,
                 stream=None), fwd_only(OP_SIZES)),
        "op_bwd": Entry(
            "dstd_dstdgc_train_bwd_r",
            ("mode x B cin cout T V red w alpha saved saved_bytes dy dx g dA dalpha workspace workspace_bytes "
             "stream").split(),
            dict(OP_SHAPE, x=PTR, w=fill(native.GCWeights()), alpha=PTR, saved=PTR, saved_bytes=SHORT, dy=PTR, dx=PTR,
                 g=fill(native.GCGrads()), dA=PTR, dalpha=PTR, workspace=PTR, workspace_bytes=FULL, stream=None),
            OP_SIZES, accepted=["dx"]),
        "block_fwd": Entry(
            "dstd_block_train_fwd_ex", "p x B T V momentum y saved saved_bytes stream flags".split(),
            dict(p=block_params(6, 64), x=PTR, B=2, T=4, V=3, momentum=0.1, y=PTR, saved=PTR, saved_bytes=SHORT,
                 stream=None, flags=0), fwd_only(BLK_SIZES)),
        "block_bwd": Entry(
            "dstd_block_train_bwd_ex",
            "p x B T V saved saved_bytes dy dx g workspace workspace_bytes stream flags".split(),
            dict(p=block_params(6, 64), x=PTR, B=2, T=4, V=3, saved=PTR, saved_bytes=SHORT, dy=PTR, dx=PTR,
                 g=fill(native.BlockGrads()), workspace=PTR, workspace_bytes=FULL, stream=None, flags=0),
            BLK_SIZES, accepted=["dx"]),
        "model_fwd": Entry(
            "dstd_model_train_fwd_sync",
            "p x B momentum dropout_p seed y saved saved_bytes stream flags sync".split(),
            dict(p=model_params(4, 3, 64, MODEL_L), x=PTR, B=2, momentum=0.1, dropout_p=0.1, seed=1234, y=PTR,
                 saved=PTR, saved_bytes=SHORT, stream=None, flags=0, sync=None),
            fwd_only(MDL_SIZES), accepted=ENC_RES),
        "model_bwd": Entry(
            "dstd_model_train_bwd_sync",
            "p x B dropout_p seed saved saved_bytes dy g dx workspace workspace_bytes stream flags sync".split(),
            dict(p=model_params(4, 3, 64, MODEL_L), x=PTR, B=2, dropout_p=0.1, seed=1234, saved=PTR,
                 saved_bytes=SHORT, dy=PTR, g=model_grads(MODEL_L), dx=PTR, workspace=PTR, workspace_bytes=FULL,
                 stream=None, flags=0, sync=None),
            MDL_SIZES, accepted=ENC_RES + ["dx"]),
    }


# ---------------------------------------------------------------------------
# rows: (label, {path: value}, expected code)
# ---------------------------------------------------------------------------
def null_rows(e, names):
    """Each pointer argument, and each pointer member of each structure argument,
    NULL in turn: -1, or still the base's -2 where NULL is accepted."""
    rows = []
    for k in names:
        v = e.base[k]
        paths = [k] + (list(leaves(v, k)) if isinstance(v, ctypes.Structure) else [])
        for path in paths:
            if beyond_layers(path):
                continue
            rows.append((f"{path} NULL", {path: None}, EWORKSPACE if path in e.accepted else EINVAL))
    return rows


def size_rows(e):
    rows = []
    for k in e.sizes:
        ch = {s: FULL for s in e.sizes}
        ch[k] = SHORT
        if any(e.base[s] != v for s, v in ch.items()):  # (a forward's only size: the base row itself)
            rows.append((f"{k} = export - 1", ch, EWORKSPACE))
    return rows


def op_rows(e, bwd):
    ptrs = ["x", "w", "alpha", "saved"] + (["dy", "dx", "g", "dA", "dalpha", "workspace"] if bwd else ["A", "y"])
    rows = null_rows(e, ptrs) + size_rows(e)
    rows += [("mode 2", {"mode": 2}, EINVAL), ("B = 0", {"B": 0}, EINVAL), ("T = 1", {"T": 1}, EINVAL),
             ("V = 0", {"V": 0}, EINVAL), ("red = 0", {"red": 0}, EINVAL),
             ("T = 129", {"T": 129}, ELIMIT), ("V = 33", {"V": 33}, ELIMIT), ("cin = 0", {"cin": 0}, ELIMIT),
             ("cin = 65", {"cin": 65}, ELIMIT), ("cout = 0", {"cout": 0}, ELIMIT), ("cout = 65", {"cout": 65}, ELIMIT),
             ("red = 9", {"red": 9}, ELIMIT),
             ("temporal mode", {"mode": 1}, EWORKSPACE),
             ("x NULL and T = 129", {"x": None, "T": 129}, EINVAL),
             ("T = 129 and saved_bytes = 0", {"T": 129, "saved_bytes": 0}, ELIMIT)]
    return rows


def block_rows(e, bwd):
    ptrs = ["p", "x", "saved"] + (["dy", "dx", "g", "workspace"] if bwd else ["y"])
    rows = null_rows(e, ptrs) + size_rows(e)
    rows += [("B = 0", {"B": 0}, EINVAL), ("T = 1", {"T": 1}, EINVAL), ("V = 0", {"V": 0}, EINVAL),
             ("unknown flag 4", {"flags": 4}, EINVAL), ("PAIRED with odd B", {"flags": 2, "B": 3}, EINVAL),
             ("PAIRED with even B", {"flags": 2}, EWORKSPACE), ("RUNNING_STATS", {"flags": 1}, EWORKSPACE),
             ("T = 129", {"T": 129}, ELIMIT), ("V = 33", {"V": 33}, ELIMIT),
             ("x NULL and T = 129", {"x": None, "T": 129}, EINVAL),
             ("T = 129 and saved_bytes = 0", {"T": 129, "saved_bytes": 0}, ELIMIT)]
    # the training block_ok range-checks the channels itself: -1 where the eval forward says -3
    rows += [(f"{k} = {v}", {f"p.{k}": v}, EINVAL) for k in ("cin", "cout") for v in (0, 65)]
    # cin == cout: the residual members are not wanted
    same = {"p.cin": 64, "p.res_w": None, "p.res_b": None, "p.res_bn.weight": None, "p.res_bn.bias": None,
            "p.res_bn.running_mean": None, "p.res_bn.running_var": None}
    if bwd:
        same.update({"g.res_w": None, "g.res_b": None, "g.res_bn.weight": None, "g.res_bn.bias": None})
    rows.append(("cin == cout without the residual members", same, EWORKSPACE))
    return rows


def model_rows(e, bwd):
    ptrs = ["p", "x", "saved"] + (["dy", "g", "dx", "workspace"] if bwd else ["y"])
    rows = null_rows(e, ptrs) + size_rows(e)
    nan = float("nan")
    rows += [("B = 0", {"B": 0}, EINVAL), ("T = 1", {"p.T": 1}, EINVAL), ("V = 0", {"p.V": 0}, EINVAL),
             ("unknown flag 16", {"flags": 16}, EINVAL), ("PAIRED with odd B", {"flags": 2, "B": 3}, EINVAL),
             ("every known flag", {"flags": 15, "seed": PTR}, EWORKSPACE),
             ("dropout_p = -0.1", {"dropout_p": -0.1}, EINVAL), ("dropout_p = 1.0", {"dropout_p": 1.0}, EINVAL),
             ("dropout_p = NaN", {"dropout_p": nan}, EINVAL), ("dropout_p = 0", {"dropout_p": 0.0}, EWORKSPACE),
             ("SEED_DEVICE, dropout_p > 0, seed 0", {"flags": 4, "seed": 0}, EINVAL),
             ("SEED_DEVICE, dropout_p = 0, seed 0", {"flags": 4, "seed": 0, "dropout_p": 0.0}, EWORKSPACE),
             ("num_layers = -1", {"p.num_layers": -1}, EINVAL), ("num_layers = 17", {"p.num_layers": 17}, EINVAL),
             ("in_channels = 3", {"p.in_channels": 3}, EINVAL),
             ("sync", {"sync": bn_sync()}, EWORKSPACE),
             ("sync with fn NULL", {"sync": bn_sync(), "sync.fn": _NULL_FN}, EINVAL),
             ("sync with buf NULL", {"sync": bn_sync(), "sync.buf": None}, EINVAL),
             ("sync with world = 0", {"sync": bn_sync(), "sync.world": 0}, EINVAL),
             ("sync with rank = world", {"sync": bn_sync(), "sync.rank": 2}, EINVAL),
             ("sync with rank = -1", {"sync": bn_sync(), "sync.rank": -1}, EINVAL),
             ("sync with buf_floats one short", {"sync": bn_sync(), "sync.buf_floats": bn_sync().buf_floats - 1},
              EINVAL),
             ("T = 129", {"p.T": 129}, ELIMIT), ("V = 33", {"p.V": 33}, ELIMIT),
             # ch_ok(num_feature) answers before the blocks' channels are compared with it
             ("num_feature = 65 with 64-channel blocks", {"p.num_feature": 65}, ELIMIT),
             # ... but blocks that follow it to 65 are refused by the training block_ok first
             ("num_feature = 65 with 65-channel blocks",
              {"p.num_feature": 65, "p.st_in.cout": 65, "p.enc.0.cin": 65, "p.enc.0.cout": 65, "p.st_out.cin": 65},
              EINVAL),
             ("x NULL and T = 129", {"x": None, "p.T": 129}, EINVAL),
             ("T = 129 and saved_bytes = 0", {"p.T": 129, "saved_bytes": 0}, ELIMIT)]
    rows += [(f"{b}.{k} = {v}", {f"p.{b}.{k}": v}, EINVAL) for b in ("st_in", "enc.0", "st_out")
             for k in ("cin", "cout") for v in (0, 65)]
    # only the forward compares the end blocks' channels with num_feature / 6 / 3
    ends = [("st_in.cin", 5), ("st_in.cout", 32), ("st_out.cin", 32), ("st_out.cout", 4)]
    rows += [(f"{k} = {v}", {f"p.{k}": v}, EWORKSPACE if bwd else EINVAL) for k, v in ends]
    if bwd:  # the gradient pointers are looked at after the envelope
        rows.append(("g.prelu NULL and T = 129", {"g.prelu": None, "p.T": 129}, ELIMIT))
    return rows


ROWS = {"op_fwd": lambda e: op_rows(e, False), "op_bwd": lambda e: op_rows(e, True),
        "block_fwd": lambda e: block_rows(e, False), "block_bwd": lambda e: block_rows(e, True),
        "model_fwd": lambda e: model_rows(e, False), "model_bwd": lambda e: model_rows(e, True)}
# (a table that lost its generated NULL rows would still pass: the counts are held)
NUM_ROWS = {"op_fwd": 29, "op_bwd": 42, "block_fwd": 62, "block_bwd": 102, "model_fwd": 184, "model_bwd": 303}


def build_row(e, changes, want):
    """The row's arguments, after checking that the call cannot pass every
    check: it differs from the base in a field that is refused, or (where -2 is
    expected) carries a size below the export for its own shape."""
    a = clone(e.base)
    for path, v in changes.items():
        set_path(a, path, v)
    changed = [p for p in changes if differs(a, e.base, p)]
    assert changed, "the row does not differ from the base row"
    if want == EWORKSPACE:
        # sized for the row's own shape, which reaches the size checks
        a = e.resolve(a, a)
        assert any(a[k] < ex for k, ex in e.exports(a).items()), "no size argument is short"
    else:
        # refused before the sizes are looked at: the base shape's will do
        a = e.resolve(a, e.base)
        assert any(p not in e.accepted and p not in e.sizes for p in changed) or "saved_bytes" in changes
    return a


@pytest.mark.parametrize("name", sorted(ROWS))
def test_training_entry_point_refusals(name):
    e = entries()[name]
    base = e.resolve(clone(e.base), e.base)
    assert base["saved_bytes"] == e.exports(base)["saved_bytes"] - 1
    assert e.call(base) == EWORKSPACE, "the base row must pass everything but the size check"
    rows = ROWS[name](e)
    assert len(rows) == NUM_ROWS[name] and len({r[0] for r in rows}) == len(rows)
    wrong = []
    for label, changes, want in rows:
        assert want in (EINVAL, EWORKSPACE, ELIMIT), label  # no row may be accepted
        got = e.call(build_row(e, changes, want))
        if got != want:
            wrong.append((label, got, want))
    assert not wrong, f"{name}: (row, returned, expected) {wrong}"


def test_wrappers_share_the_refusals():
    """The plain and _ex entry points are the _r / _ex / _sync ones with
    red = 2, flags = 0 and no sync, so a refused row is refused there too."""
    L, E = native.lib(), entries()
    a = E["op_fwd"].resolve(clone(E["op_fwd"].base), E["op_fwd"].base)
    a["saved_bytes"] = int(L.dstd_dstdgc_train_saved_bytes(0, 2, 5, 7, 4, 3)) - 1
    w = ctypes.byref(a["w"])
    assert L.dstd_dstdgc_train_fwd(0, PTR, 2, 5, 7, 4, 3, w, PTR, PTR, PTR, PTR, a["saved_bytes"], None) == EWORKSPACE
    assert L.dstd_dstdgc_train_fwd(0, PTR, 2, 5, 7, 129, 3, w, PTR, PTR, PTR, PTR, a["saved_bytes"], None) == ELIMIT
    b = E["block_fwd"].resolve(clone(E["block_fwd"].base), E["block_fwd"].base)
    p = ctypes.byref(b["p"])
    assert L.dstd_block_train_fwd(p, PTR, 2, 4, 3, 0.1, PTR, PTR, b["saved_bytes"], None) == EWORKSPACE
    assert L.dstd_block_train_fwd(p, PTR, 2, 4, 33, 0.1, PTR, PTR, b["saved_bytes"], None) == ELIMIT
    m = E["model_bwd"].resolve(clone(E["model_bwd"].base), E["model_bwd"].base)
    mp, mg = ctypes.byref(m["p"]), ctypes.byref(m["g"])
    assert L.dstd_model_train_bwd(mp, PTR, 2, 0.1, 1234, PTR, m["saved_bytes"], PTR, mg, PTR, m["workspace_bytes"],
                                  None) == EWORKSPACE
    assert L.dstd_model_train_bwd_ex(mp, PTR, 2, 0.1, 1234, PTR, m["saved_bytes"], PTR, mg, None, PTR,
                                     m["workspace_bytes"], None, 16) == EINVAL
