"""Read the public headers (include/*.h) with `re` and compare them with the
ctypes binding (dstd_native.abi).  Knows the C these headers use, no more:
comments, preprocessor lines, integer defines, struct typedefs with comma
declarators and array fields, one function-pointer typedef, prototypes."""
import ctypes
import re

TYPE_WORDS = {"unsigned", "long", "int", "float", "char", "void", "size_t", "short", "double"}
SCALARS = {"int": ctypes.c_int, "unsigned int": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}


def _decl(text):
    """'const float* const* x[N]' -> (base 'float', pointer depth 2, name 'x', array 'N' or None)."""
    m = re.search(r"\[\s*(\w+)\s*\]\s*$", text)
    array = m.group(1) if m else None
    tokens = [t for t in re.findall(r"\w+|\*", text[:m.start()] if m else text) if t != "const"]
    words = [t for t in tokens if t != "*"]
    name = words.pop() if len(words) > 1 and words[-1] not in TYPE_WORDS else None
    base = " ".join(words)
    return {"unsigned": "unsigned int", "long long int": "long long"}.get(base, base), tokens.count("*"), name, array


def _params(text):
    text = text.strip()
    return [] if text in ("", "void") else [_decl(a)[:3] for a in text.split(",")]


def parse(text):
    """One header -> (defines {name: value text}, structs {name: [(field, base, depth, array)]},
    callbacks {name: (ret, params)}, prototypes {name: (ret, params)}); ret and each
    param are (base, depth[, name])."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    defines = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DSTD_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)  # before prototypes: a return type must not swallow one
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs, callbacks = {}, {}
    for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for stmt in filter(str.strip, m.group(1).split(";")):
            first, *more = stmt.split(",")
            base, depth, name, array = _decl(first)
            fields.append((name, base, depth, array))
            for d in more:  # `int cin, cout;`: the base type once, pointer depth and array per declarator
                _, depth, name, array = _decl("int " + d)
                fields.append((name, base, depth, array))
        structs[m.group(2)] = fields
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
    for m in re.finditer(r"typedef\s+([^;()]+?)\(\s*\*\s*(\w+)\s*\)\s*\(([^()]*)\)\s*;", text):
        callbacks[m.group(2)] = (_decl(m.group(1) + " _")[:2], _params(m.group(3)))
    text = re.sub(r"typedef[^;]*;", " ", text)
    protos = {m.group(2): (_decl(m.group(1) + " _")[:2], _params(m.group(3)))
              for m in re.finditer(r"([^;{}()]+?)\b(dstd_\w+)\s*\(([^()]*)\)\s*;", text)}
    return defines, structs, callbacks, protos


def int_defines(defines):
    """{name: int} of the defines whose value is an integer literal (sign, hex,
    u / l suffixes, parentheses) or another such define."""
    out = {}

    def value(v, seen=()):
        v = v.strip("() \t")
        m = re.fullmatch(r"([-+]?)\s*(0[xX][0-9a-fA-F]+|\d+)[uUlL]*", v)
        if m:
            return int(m.group(1) + m.group(2), 0)
        return value(defines[v], seen + (v,)) if v in defines and v not in seen else None

    for k, v in defines.items():
        n = value(v)
        if n is not None:
            out[k] = n
    return out


def _is_pointer(t):
    return isinstance(t, type) and issubclass(t, ctypes._Pointer)


def _matches(base, depth, py, types, ret=False):
    if depth == 0:
        return py is (types[base] if base in types else SCALARS.get(base, ()))
    if depth == 1 and base in types:  # a mirrored struct: by class
        return py is ctypes.POINTER(types[base])
    if ret and (base, depth) == ("char", 1):
        return py is ctypes.c_char_p
    if py is ctypes.c_void_p:
        return True
    # POINTER(X): X matches what the C pointer points to (a plain void* is c_void_p alone)
    return _is_pointer(py) and (depth > 1 or base != "void") and _matches(base, depth - 1, py._type_, types)


def _c(base, depth):
    return base + "*" * depth


def _py(t):
    return getattr(t, "__name__", repr(t))


def _signature(name, where, c_sig, restype, argtypes, types, out):
    (rb, rd), params = c_sig
    if not _matches(rb, rd, restype, types, ret=True):
        out.append(f"{name}: returns {_c(rb, rd)} in {where}, {_py(restype)} in the binding")
    if len(params) != len(argtypes):
        out.append(f"{name}: {len(params)} parameters in {where}, {len(argtypes)} in the binding")
        return
    for k, ((b, d, pname), t) in enumerate(zip(params, argtypes)):
        if not _matches(b, d, t, types):
            out.append(f"{name}: parameter {k} ({pname}) is {_c(b, d)} in {where}, {_py(t)} in the binding")


def compare(headers, binding):
    """headers: {file name: text}.  binding: the namespace that holds ABI,
    C_TYPES and the constants.  Returns the disagreements, each a line that
    starts with the C name it is about; empty when the two agree."""
    out = []
    parsed = {h: parse(t) for h, t in headers.items()}
    defines = {k: v for p in parsed.values() for k, v in p[0].items()}
    structs = {k: v for p in parsed.values() for k, v in p[1].items()}
    callbacks = {k: v for p in parsed.values() for k, v in p[2].items()}
    ints = int_defines(defines)
    types = dict(binding.C_TYPES)

    # functions
    for h in sorted(set(parsed) | set(binding.ABI)):
        protos, table = parsed.get(h, ({},) * 4)[3], binding.ABI.get(h, {})
        for name in sorted(set(protos) - set(table)):
            out.append(f"{name}: declared in {h}, absent from the binding's table for it")
        for name in sorted(set(table) - set(protos)):
            out.append(f"{name}: in the binding's table for {h}, not declared there")
        for name in sorted(set(protos) & set(table)):
            _signature(name, h, protos[name], table[name][0], table[name][1], types, out)
    names = [n for t in binding.ABI.values() for n in t]
    for name in sorted({n for n in names if names.count(n) > 1}):
        out.append(f"{name}: more than once in the binding's table")

    # structs and the callback typedef
    for name in sorted((set(structs) | set(callbacks)) - set(types)):
        out.append(f"{name}: typedef in the headers, absent from C_TYPES")
    for name in sorted(set(types) - set(structs) - set(callbacks)):
        out.append(f"{name}: in C_TYPES, no such typedef in the headers")
    classes = {v for v in vars(binding).values() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    for cls in sorted(classes - set(types.values()), key=_py):
        out.append(f"{_py(cls)}: a Structure of the binding that C_TYPES maps to no typedef")
    for name in sorted(set(callbacks) & set(types)):
        _signature(name, "its typedef", callbacks[name], types[name]._restype_, types[name]._argtypes_, types, out)
    for name in sorted(set(structs) & set(types)):
        cls, fields = types[name], structs[name]
        if "_pack_" in vars(cls):
            out.append(f"{name}: {_py(cls)} sets _pack_")
        if [f[0] for f in fields] != [f[0] for f in cls._fields_]:
            out.append(f"{name}: fields {[f[0] for f in fields]} in the header, "
                       f"{[f[0] for f in cls._fields_]} in {_py(cls)}")
            continue
        for (fname, base, depth, array), (_, t) in zip(fields, cls._fields_):
            if array is not None:
                n = int(array) if array.isdigit() else ints.get(array)
                if getattr(t, "_length_", None) != n:
                    out.append(f"{name}: field {fname} has {array} = {n} elements in the header, "
                               f"{getattr(t, '_length_', 'no')} in {_py(cls)}")
                    continue
                t = t._type_
            elif hasattr(t, "_length_"):
                out.append(f"{name}: field {fname} is no array in the header, {_py(t)} in {_py(cls)}")
                continue
            if not _matches(base, depth, t, types):
                out.append(f"{name}: field {fname} is {_c(base, depth)} in the header, {_py(t)} in {_py(cls)}")

    # constants: DSTD_X <-> X
    for name, value in sorted(ints.items()):
        got = getattr(binding, name[len("DSTD_"):], None)
        if type(got) is not int or got != value:
            out.append(f"{name}: {value} in the headers, {name[len('DSTD_'):]} = {got!r} in the binding")
    return out
