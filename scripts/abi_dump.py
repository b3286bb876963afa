"""Print the ctypes binding as the loaded library carries it: every exported
entry point's restype and argtypes, every Structure's fields with offset and
size.  Two revisions marshal calls alike iff their dumps are equal
(profiles/r15_abi_binding_*.txt)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dstd-gcn_amd"))
import dstd_native as native  # noqa: E402


def tname(t):
    if t is None:
        return "None"
    if hasattr(t, "_length_"):
        return f"{tname(t._type_)}[{t._length_}]"
    if hasattr(t, "_argtypes_"):
        return f"{tname(t._restype_)}(*)({', '.join(tname(a) for a in t._argtypes_)})"
    if isinstance(getattr(t, "_type_", None), type):
        return f"POINTER({tname(t._type_)})"
    return t.__name__


def main():
    L = native.lib()
    names = [n for k in sorted(vars(native)) if k.endswith("EXPORTS") for n in getattr(native, k)]
    for n in sorted(names):
        fn = getattr(L, n)
        args = "None" if fn.argtypes is None else "[" + ", ".join(tname(a) for a in fn.argtypes) + "]"
        print(f"fn {n}: {tname(fn.restype)} {args}")
    print(f"callback COLLECTIVE_FN: {tname(native.COLLECTIVE_FN)}")
    structs = {k: v for k, v in vars(native).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    for k in sorted(structs):
        s = structs[k]
        print(f"struct {k}: size {ctypes.sizeof(s)} align {ctypes.alignment(s)}")
        for name, t in s._fields_:
            d = getattr(s, name)
            print(f"  {name}: {tname(t)} offset {d.offset} size {d.size}")


if __name__ == "__main__":
    main()
