"""ctypes binding of the fnoengine C ABI, derived from include/fnoengine.h when this module is imported: constants, structs,
the symbol list and every function's types are read from the header (read_header), never written out a second time.

The shared library is built in-tree by `python -m pde_policylearning_amd.build`
(or __graft_entry__.build()) with hipcc for gfx950.  There is NO fallback: if
the library is missing or a call fails, a RuntimeError is raised.
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FNO_LIB_PATH") or os.path.join(_HERE, "libfnoengine.so")      # (FNO_LIB_PATH: experiment builds of tools/)

Header = collections.namedtuple("Header", "consts structs protos")

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
            "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}


def _ctype(text, where, structs, opaque, role):
    """The ctypes type of the C type `text` as a return type, argument or struct field (role "ret" / "arg" / "field").
    A type outside the rules below raises, naming `where`: nothing defaults to a pointer or an int."""
    words = re.findall(r"[A-Za-z_]\w*", text)
    base, stars = " ".join(w for w in words if w != "const"), text.count("*")
    bad = RuntimeError(f"fnoengine header: {where}: unknown type '{' '.join(text.split())}'")
    if re.sub(r"[\w\s*]", "", text):
        raise bad
    if stars == 0:
        if base in _SCALARS:
            return _SCALARS[base]
        if base == "void" and role == "ret":
            return None
        raise bad
    if stars > 2 or not (base in _SCALARS or base in ("void", "char") or base in structs or base in opaque):
        raise bad
    if role == "ret":
        if words == ["const", "char"] and stars == 1:
            return C.c_char_p
        raise bad
    if role == "field":
        return C.c_void_p
    if stars == 1:
        return C.POINTER(structs[base]) if base in structs else C.c_void_p
    if base in opaque or re.search(r"\*\s*const\s*\*", text):       # plan out-parameters; tables of device pointers
        return C.POINTER(C.c_void_p)
    return C.c_void_p


def read_header(text, consts=None, structs=None):
    """Header(consts, structs, protos) of a C header in the style of include/fnoengine.h: every `#define NAME integer` and
    enumerator of an anonymous enum; every `typedef struct Name {...} Name;` as a ctypes.Structure (pointer fields as
    c_void_p); every prototype as name -> (restype, argtypes), in header order.  `consts` / `structs` carry the names of a
    header read before.  Whatever the reader does not recognise raises, naming the function and parameter or the field."""
    consts, structs, opaque, protos = dict(consts or {}), dict(structs or {}), set(), {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M):
        consts[name] = int(value)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', " ", text)

    def enum(m):
        value = -1
        for item in filter(None, (i.strip() for i in m.group(1).split(","))):
            em = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\d+))?", item)
            if not em:
                raise RuntimeError(f"fnoengine header: cannot read the enumerator '{item}'")
            value = int(em.group(2)) if em.group(2) else value + 1
            consts[em.group(1)] = value
        return " "

    def struct(m):
        body, sname = m.groups()
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            fm = re.fullmatch(r"(.*?)(\w+)((?:\s*\[\s*\w+\s*\])*)", first, re.S)
            rest = [re.fullmatch(r"()(\w+)((?:\s*\[\s*\w+\s*\])*)", d) for d in more]
            if not fm or not all(rest) or (more and "*" in fm.group(1)):
                raise RuntimeError(f"fnoengine header: {sname}: cannot place the field '{' '.join(decl.split())}'")
            ctype = _ctype(fm.group(1), f"{sname}.{fm.group(2)}", structs, opaque, "field")
            for dm in [fm] + rest:
                t = ctype
                for dim in reversed(re.findall(r"\w+", dm.group(3))):
                    if not (dim.isdigit() or dim in consts):
                        raise RuntimeError(f"fnoengine header: {sname}.{dm.group(2)}: unknown extent '{dim}'")
                    t = t * (int(dim) if dim.isdigit() else consts[dim])
                fields.append((dm.group(2), t))
        structs[sname] = type(sname, (C.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    *statements, tail = text.split(";")

    def unreadable(stmt):
        m = re.search(r"(\w+)\s*\(", stmt)
        return RuntimeError(f"fnoengine header: cannot read the declaration of '{m.group(1) if m else ' '.join(stmt.split())[:60]}'")

    for stmt in statements:
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        om = re.fullmatch(r"typedef struct (\w+) (\w+)", stmt)
        if om:
            opaque.add(om.group(2))
            continue
        pm = re.fullmatch(r"([^()]*?)(\w+) ?\(([^()]*)\)", stmt)
        if not pm or pm.group(2) in protos:
            raise unreadable(stmt)
        ret, name, params = pm.groups()
        args = []
        for prm in [] if params.strip() == "void" else params.split(","):
            am = re.fullmatch(r"(.*?)(\w+)", prm.strip())
            if not am:
                raise RuntimeError(f"fnoengine header: {name}: cannot read the parameter '{prm.strip()}'")
            args.append(_ctype(am.group(1), f"{name}({am.group(2)})", structs, opaque, "arg"))
        protos[name] = (_ctype(ret, name, structs, opaque, "ret"), args)
    if tail.split() != ["}"] * n_extern:          # what follows the last `;` is the closing brace of extern "C" and nothing else
        raise unreadable(tail)
    return Header(consts, structs, protos)


def _header(path, *before):
    if not os.path.exists(path):
        raise RuntimeError(f"fnoengine: {path} not found: the binding is derived from it (there is no second copy of the ABI).")
    with open(path) as f:
        return read_header(f.read(), *before)


# The ABI is stated once, in the header (the compiler holds csrc/fno_abi.hip to it); everything below is read from it.
ABI = _header(os.path.join(os.path.dirname(_HERE), "include", "fnoengine.h"))
DEBUG_ABI = _header(os.path.join(_HERE, "csrc", "fno_debug.h"), ABI.consts, ABI.structs)     # not public: bound where defined
globals().update(ABI.structs)          # FnoSpecDesc, FnoModelDesc, FnoModelParams, FnoModelGrads, FnoBlockTail, ...
EXPORTED_SYMBOLS = list(ABI.protos)
FNO_MAX_LAYERS = ABI.consts["FNO_MAX_LAYERS"]
FNO_CTRL_STATS_MAX = ABI.consts["FNO_CTRL_STATS_MAX"]
NORM_CODES = {"backward": ABI.consts["FNO_NORM_BACKWARD"], None: ABI.consts["FNO_NORM_BACKWARD"],
              "forward": ABI.consts["FNO_NORM_FORWARD"], "ortho": ABI.consts["FNO_NORM_ORTHO"]}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"fnoengine: {LIB_PATH} not found. Build it with `python -m pde_policylearning_amd.build` "
            "(needs hipcc; gfx950). There is no CPU / PyTorch fallback.")
    # torch first: its wheel carries its own libamdhip64.so.7 / libhsa-runtime64, and the library works on pointers torch's
    # allocator hands out, so both must sit on ONE HIP runtime.  Loaded after torch, the library's NEEDED libamdhip64.so.7
    # resolves to the copy already in the process; loaded before it, /opt/rocm's copy comes in as a second runtime and
    # every later call fails with "no HIP device" (seen with build() and smoke() in one process).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    missing = [n for n in ABI.protos if not hasattr(L, n)]
    if missing:
        raise RuntimeError(f"fnoengine: {LIB_PATH} does not define {missing} (include/fnoengine.h declares them): rebuild it.")
    for name, (restype, argtypes) in list(ABI.protos.items()) + [p for p in DEBUG_ABI.protos.items() if hasattr(L, p[0])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().fno_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"fnoengine {what} failed (code {rc}): {msg}")


def profile_summary(with_terms=False):
    """[(kernel name, total ms, launches)] recorded since the last reset (profiling on); with_terms: a fourth entry, the
    matrix pipe of the kernel's channel GEMMs (fno_profile_get_terms: 0 not stated, 1 fp32, 2 two fp16 terms, 3 three bf16)."""
    L = lib()
    out = []
    for i in range(L.fno_profile_count()):
        name, ms, n = C.c_char_p(), C.c_float(), C.c_int()
        L.fno_profile_get(i, C.byref(name), C.byref(ms), C.byref(n))
        rec = (name.value.decode(), float(ms.value), int(n.value))
        out.append(rec + (int(L.fno_profile_get_terms(i)),) if with_terms else rec)
    return out


class launch_log(object):
    """`with launch_log() as log:` records every kernel launch of the library inside the block (fno_debug_launch_log: made by
    the launching statement itself, off by default); afterwards `log.records` is a list of dicts
    {"name": profile label, "variant": the dispatch site's tag (kernel and template arguments, "" where it states none),
     "rb", "ntiles" (0 where the site has none), "grid", "block" (3-tuples), "lds" (bytes)} in launch order."""

    def __enter__(self):
        self.records = []
        lib().fno_debug_launch_log(1)
        return self

    def __exit__(self, *exc):
        L = lib()
        try:
            for i in range(L.fno_debug_launch_count()):
                name, var, rb, nt, lds = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int(), C.c_size_t()
                grid, block = (C.c_uint * 3)(), (C.c_uint * 3)()
                check(L.fno_debug_launch_get(i, C.byref(name), C.byref(var), C.byref(rb), C.byref(nt), grid, block, C.byref(lds)),
                      "debug_launch_get")
                self.records.append({"name": name.value.decode(), "variant": var.value.decode(), "rb": int(rb.value),
                                     "ntiles": int(nt.value), "grid": tuple(grid), "block": tuple(block), "lds": int(lds.value)})
        finally:
            L.fno_debug_launch_log(0)
        return False
