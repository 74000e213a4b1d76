"""CPU: the binding table of 3dfacerecon_amd/_lib.py (SIGNATURES) against the prototypes of include/fr_hotpath.h -- the same
names, and for each the same number of parameters with the same ABI class in every position and for the return value.  The
library is bound from the table alone, so a row that disagrees with the header would be a garbage call; this is the one place
that compares them."""
import os
import re

from conftest import ROOT, pkg

_ABI = {"int": "int", "size_t": "size_t", "unsigned long long": "unsigned long long", "float": "float", "double": "double",
        "void": "void"}
_CODE = {"p": "pointer", "s": "pointer", "I": "pointer", "D": "pointer", "i": "int", "z": "size_t", "u": "unsigned long long",
         "f": "float", "d": "double", "v": "void"}


def _abi_class(ctype):
    if "*" in ctype:
        return "pointer"
    words = " ".join(w for w in ctype.split() if w != "const")
    assert words in _ABI, "a type this test does not know: %r" % ctype
    return _ABI[words]


def _header_prototypes():
    """-> {name: (return class, [parameter classes])} of every `ret name(args);` in the header, comments stripped"""
    src = open(os.path.join(ROOT, "include", "fr_hotpath.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_0-9\s\*]*?)\b(fr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in protos, "declared twice: " + name
        params = []
        for a in (a.strip() for a in args.split(",")):
            if a in ("", "void"):
                assert args.strip() in ("", "void")
                continue
            m = re.match(r"^(.*?)(\w+)$", a, flags=re.S)   # the last word is the parameter's name
            assert m and m.group(1).strip(), "unnamed parameter in %s: %r" % (name, a)
            params.append(_abi_class(m.group(1)))
        protos[name] = (_abi_class(ret), params)
    # nothing that looks like a declaration of an entry point escaped the pattern above
    assert sorted(protos) == sorted(set(re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", src)))
    return protos


def test_binding_table_matches_every_header_prototype():
    host = pkg("_lib")
    protos = _header_prototypes()
    assert len(protos) >= 69
    assert sorted(host.SIGNATURES) == sorted(protos) and len(host.SIGNATURES) == len(protos)
    assert list(host.EXPORTS) == list(host.SIGNATURES)
    for name, sig in host.SIGNATURES.items():
        ret, args = sig.split(":")
        want_ret, want_args = protos[name]
        assert len(ret) == 1 and _CODE[ret] == want_ret, (name, "return", ret, want_ret)
        assert len(args) == len(want_args), (name, len(args), len(want_args))
        for k, (c, want) in enumerate(zip(args, want_args)):
            assert _CODE[c] == want, (name, "parameter %d" % k, c, want)
        assert set(ret + args) <= set(host._CTYPE), name


def test_bind_sets_the_python_visible_types():
    """bind() on a stand-in object: every row becomes restype / argtypes, with today's Python-visible types for the hooks'
    `int* out`, the option names and the float / double scalars"""
    import ctypes
    import types
    host = pkg("_lib")

    class Fake:
        def __getattr__(self, k):
            v = types.SimpleNamespace()
            object.__setattr__(self, k, v)
            return v
    L = host.bind(Fake())
    assert sorted(vars(L)) == sorted(host.SIGNATURES)
    assert L.fr_version.restype is ctypes.c_char_p and L.fr_version.argtypes == []
    assert L.fr_get_option.argtypes == [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    assert L.fr_debug_sfs_geom.restype is None and L.fr_debug_sfs_geom.argtypes[-1] is ctypes.POINTER(ctypes.c_int)
    assert L.fr_debug_sfs_pinv.argtypes == [ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_int)]
    assert L.fr_decode_3dmm.argtypes[7] is ctypes.c_float and L.fr_sfs_solve_shade.argtypes[7] is ctypes.c_double
    assert L.fr_render_depth_workspace_bytes.restype is ctypes.c_size_t
    assert L.fr_debug_div3_sweep.argtypes[:2] == [ctypes.c_ulonglong] * 2
