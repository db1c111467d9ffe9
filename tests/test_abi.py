"""The C-ABI library loads and exports every symbol include/pinsage_hip.h declares (no compute:
runs without a GPU), and the product path fails loudly without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "pinsage_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(native.SO_PATH)
    syms = _declared_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/pinsage_hip.h but not exported"
    assert sorted(native.SYMBOLS) == syms
    lib.ps_error_string.restype = ctypes.c_char_p
    assert lib.ps_abi_version() == 1
    assert lib.ps_error_string(0) == b"ok" and b"invalid" in lib.ps_error_string(-1)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pinsage_hip import native
    from utils.random_walk import RandomWalkSampler
    from model.pinsage import ImportancePooling
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(native.NativeError):
        RandomWalkSampler(ei)
    with pytest.raises(native.NativeError):
        ImportancePooling()(torch.zeros(2, 4), [[0]], [[1.0]])


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "movie-recommendation-engine_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(d, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f


def _header_declarations():
    """{name: (return type, [parameter declarations])} as include/pinsage_hip.h writes them"""
    txt = open(os.path.join(ROOT, "include", "pinsage_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(ps_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S):
        params = params.strip()
        out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [" ".join(q.split()) for q in params.split(",")])
    return out


def _header_arity():
    return {name: len(params) for name, (_, params) in _header_declarations().items()}


_SCALARS = {"int": "i", "int64_t": "q", "size_t": "z", "uint64_t": "Q", "uint32_t": "I", "float": "f"}


def _code(ctype):
    """the letter native.PROTOTYPES uses for a C type: every pointer and ps_stream_t is `p` (`s` for the returned string)"""
    ctype = ctype.replace("const ", "").strip()
    if "*" in ctype:
        return "s" if ctype.startswith("char") else "p"
    return "p" if ctype == "ps_stream_t" else _SCALARS[ctype]


def test_prototypes_equal_the_header():
    from pinsage_hip import native
    decl = _header_declarations()
    assert sorted(decl) == _declared_symbols() == sorted(native.PROTOTYPES) and len(decl) >= 50
    assert native.SYMBOLS == list(native.PROTOTYPES)
    for name, (ret, params) in decl.items():
        # a parameter is "<type> <name>"; the `*` of a pointer may stand on either side of the blank
        want = [_code(q if "*" in q else q.rsplit(" ", 1)[0]) for q in params]
        got_ret, _, got = native.PROTOTYPES[name].partition(" ")
        assert got_ret == _code(ret), f"{name}: returns {ret}, table says {got_ret!r}"
        assert len(got) == len(want), f"{name}: header declares {len(want)} parameters, table has {len(got)}"
        assert list(got) == want, f"{name}: header {''.join(want)}, table {got}"


def _lib():
    from pinsage_hip import native
    if not native.have_lib():
        import __graft_entry__ as ge
        ge.build()
    return native.lib()


def test_lib_sets_every_prototype():
    from pinsage_hip import native
    lib = _lib()
    for name, code in native.PROTOTYPES.items():
        ret, _, params = code.partition(" ")
        fn = getattr(lib, name)
        assert fn.restype is native._CTYPES[ret] and list(fn.argtypes) == [native._CTYPES[c] for c in params], name
    assert native._CTYPES == {"p": ctypes.c_void_p, "q": ctypes.c_int64, "i": ctypes.c_int, "z": ctypes.c_size_t, "Q": ctypes.c_uint64,
                              "I": ctypes.c_uint32, "f": ctypes.c_float, "s": ctypes.c_char_p}
    assert lib.ps_abi_version() == 1 and lib.ps_error_string(0) == b"ok" and b"invalid" in lib.ps_error_string(-1)


def test_high_words_arrive():
    """a plain Python int above 2^32 reaches an int64_t parameter whole (without a prototype ctypes passes it as a C int)"""
    fn = _lib().ps_lsh_planes_bytes
    big, small = fn(2 ** 33 + 2 ** 20, 64), fn(2 ** 20, 64)
    assert big != small and big > 2 ** 32
    assert big == fn(ctypes.c_int64(2 ** 33 + 2 ** 20), ctypes.c_int(64))
    raw = ctypes.CDLL(_lib()._name).ps_lsh_planes_bytes          # the same export as a call site without prototypes would see it
    raw.restype = ctypes.c_size_t
    assert big == raw(ctypes.c_int64(2 ** 33 + 2 ** 20), ctypes.c_int(64))


def test_wrong_types_are_refused():
    fn = _lib().ps_hamming_topk_mfma_workspace_bytes
    assert fn(64, 4096, 64, 10) > 0
    with pytest.raises(ctypes.ArgumentError):
        fn(64.0, 4096, 64, 10)
    with pytest.raises(ctypes.ArgumentError):
        fn(ctypes.c_int(64), 4096, 64, 10)
    with pytest.raises(ctypes.ArgumentError):
        fn(64, 4096, 64, ctypes.c_int64(10))
    with pytest.raises(TypeError):
        fn(64, 4096, 64)


def test_missing_symbol_is_named(monkeypatch):
    from pinsage_hip import native
    _lib()
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setitem(native.PROTOTYPES, "ps_not_exported", "i")
    with pytest.raises(native.NativeError, match="ps_not_exported"):
        native.lib()
    assert native._lib is None


def test_python_call_sites_pass_as_many_arguments_as_the_header_declares():
    """native.PROTOTYPES makes ctypes refuse a call with too FEW arguments, but a prototyped cdecl function takes surplus
    arguments without complaint, and the table says nothing about csrc/.  So every `nv.call("ps_x", ...)`, `lib.ps_x(...)` and
    `nv.workspace("ps_x_bytes", device, ...)` in the package (and bench/tools) is checked against the header's arity, and so
    is the C definition in csrc/ (`extern "C" ... ps_x(...)`)."""
    import ast
    arity = _header_arity()
    assert len(arity) >= 25
    checked = 0
    roots = [os.path.join(ROOT, "movie-recommendation-engine_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "bench.py"),
             os.path.join(ROOT, "__graft_entry__.py")]
    files = []
    for r in roots:
        if r.endswith(".py"):
            files.append(r)
        else:
            for d, _, fs in os.walk(r):
                files += [os.path.join(d, f) for f in fs if f.endswith(".py")]
    for f in files:
        tree = ast.parse(open(f).read())
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            fn = node.func
            if isinstance(fn, ast.Attribute) and fn.attr == "call" and node.args and isinstance(node.args[0], ast.Constant) \
                    and isinstance(node.args[0].value, str) and node.args[0].value in arity:
                name, n = node.args[0].value, len(node.args) - 1
            elif isinstance(fn, ast.Attribute) and fn.attr == "workspace" and node.args and isinstance(node.args[0], ast.Constant) \
                    and node.args[0].value in arity:
                name, n = node.args[0].value, len(node.args) - 2
            elif isinstance(fn, ast.Attribute) and fn.attr in arity:
                name, n = fn.attr, len(node.args)
            else:
                continue
            assert not any(isinstance(a, ast.Starred) for a in node.args), (f, name)
            assert n == arity[name], f"{f}: {name} called with {n} arguments, header declares {arity[name]}"
            checked += 1
    assert checked >= 30
    # the definitions
    src = ""
    csrc = os.path.join(ROOT, "movie-recommendation-engine_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith(".hip"):
            src += re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
    for name, n in arity.items():
        m = re.search(r'extern\s+"C"\s+[\w\s\*]+?\b' + name + r"\s*\(([^{;]*?)\)\s*\{", src, flags=re.S)
        assert m, f"{name} has no extern \"C\" definition"
        params = m.group(1).strip()
        got = 0 if params in ("", "void") else params.count(",") + 1
        assert got == n, f"{name}: defined with {got} parameters, declared with {n}"
