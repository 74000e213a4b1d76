"""Records what every launching C-ABI entry point returns over a grid of bad arguments: the fixture of tests/test_capi_codes_cpu.py.

    python tools/record_capi_codes.py --lib PATH/libfr_hotpath.so --out tests/golden/capi_codes.json

Run it against a library built from the commit whose behaviour is to be KEPT (the parent of a change to the argument checks), never
against the code under test, and on a machine WITHOUT a GPU: the validation code dereferences no pointer and allocates nothing, so
with no device a call that passes validation returns FR_ERR_LAUNCH (-3) -- with one, it would launch on the made-up pointers
below.  The tool refuses to run where a GPU is visible.

The grid.  Every prototype of include/fr_hotpath.h with a `hip_stream` parameter (no fr_debug_* hook) gets one valid base call
from GRID: every pointer 256 (hip_stream NULL), the ints by parameter name, the byte counts 2^40, im_size 200, rcond 1e-15.
Each argument has alternatives (pointers NULL and a misaligned 20; ints -1 and 0, and a few more by name; byte counts 0; rcond
-1 and NaN).  The cases of an entry point, in this fixed order: the base call, every single substitution (arguments left to
right, alternatives in GRID's order), every pair of substitutions on two different arguments (itertools.combinations of the
singles).  One character per case: '0' FR_OK, '1' '2' '4' the codes -1 -2 -4, '.' a call that reached HIP (not held: it
depends on the machine).  Pairs are what pins WHICH code wins when two things are wrong at once.
"""
import argparse
import ctypes
import importlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID = {
    "pointer": 256, "pointer_alts": [0, 20],
    "bytes": 1 << 40, "bytes_alts": [0],
    "im_size": 200.0,
    "rcond": 1e-15, "rcond_alts": ["-1", "nan"],
    "ints": {"B": 2, "N": 64, "nver": 64, "ntri": 5, "H": 8, "W": 8, "n_shape": 5, "n_exp": 3, "C": 3, "tex_batch": 1, "levels": 4,
             "phases": 7, "nparts": 1, "grad_stride": 3, "vertex_pitch": 64, "mode": 0, "accumulate": 0},
    "phases_decode": 15,   # `phases` of the decode -> render entry points (bit 3: the decode)
    "int_alts": [-1, 0],
    "int_more": {"H": [70000], "W": [70000], "tex_batch": [3], "levels": [3], "mode": [3], "accumulate": [3],
                 "phases": [16, 8 << 8], "ntri": [1 << 24]},
}
CHARS = {0: "0", -1: "1", -2: "2", -3: ".", -4: "4"}


def entry_points(header_text):
    """-> [(name, [parameter names])] of the launching entry points, in the header's order"""
    src = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = []
    for name, args in re.findall(r"\b(fr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        names = [re.findall(r"(\w+)$", a.strip())[0] for a in args.split(",") if a.strip() not in ("", "void")]
        if "hip_stream" in names and not name.startswith("fr_debug_"):
            out.append((name, names))
    return out


def cases(fn, names, sig, grid):
    """the argument lists of `fn`'s cases; sig = its row of _lib.SIGNATURES, names = its parameter names"""
    letters = sig.split(":")[1]
    assert len(letters) == len(names), fn
    base, singles = [], []
    for k, (c, n) in enumerate(zip(letters, names)):
        if c == "p":
            b, alts = (0, []) if n == "hip_stream" else (grid["pointer"], grid["pointer_alts"])
            conv = ctypes.c_void_p
        elif c == "z":
            b, alts, conv = grid["bytes"], grid["bytes_alts"], int
        elif c == "f":
            assert n == "im_size", (fn, n)
            b, alts, conv = grid["im_size"], [], ctypes.c_float
        elif c == "d":
            assert n == "rcond", (fn, n)
            b, alts, conv = grid["rcond"], [float(v) for v in grid["rcond_alts"]], ctypes.c_double
        elif c == "i":
            b = grid["phases_decode"] if n == "phases" and "decode" in fn else grid["ints"][n]
            alts, conv = grid["int_alts"] + grid["int_more"].get(n, []), int
        else:
            raise ValueError("%s: no base value for a %r parameter (%s)" % (fn, c, n))
        base.append(conv(b))
        singles += [(k, conv(v)) for v in alts]
    subs = [()] + [(s,) for s in singles] + [p for p in itertools.combinations(singles, 2) if p[0][0] != p[1][0]]
    for sub in subs:
        a = list(base)
        for k, v in sub:
            a[k] = v
        yield a


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the library to record: built from the commit whose return codes are to be kept")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch   # (loads the ROCm runtime the library binds to, by SONAME)
    if torch.cuda.is_available():
        raise SystemExit("record_capi_codes: a GPU is visible -- a case that passes validation would launch on made-up pointers")
    host = importlib.import_module("3dfacerecon_amd._lib")
    with open(os.path.join(ROOT, "include", "fr_hotpath.h")) as f:
        eps = entry_points(f.read())
    L = host.bind(ctypes.CDLL(os.path.abspath(args.lib)), [name for name, _ in eps] + ["fr_version"])
    funcs, total, held = {}, 0, 0
    for name, names in eps:
        f = getattr(L, name)
        codes = "".join(CHARS[f(*a)] for a in cases(name, names, host.SIGNATURES[name], GRID))
        funcs[name] = {"params": " ".join(names), "codes": codes}
        k = len(codes) - codes.count(".")
        total, held = total + len(codes), held + k
        print("%-36s %5d cases, %5.1f %% held, codes %s" % (name, len(codes), 100.0 * k / len(codes), "".join(sorted(set(codes)))))
        if k < 0.6 * len(codes):
            raise SystemExit("record_capi_codes: %s holds fewer than 60 %% of its cases" % name)
    print("%d entry points, %d cases, %d held (%.1f %%)" % (len(funcs), total, held, 100.0 * held / total))
    if held < 0.8 * total:
        raise SystemExit("record_capi_codes: fewer than 80 % of all cases held")
    with open(args.out, "w") as f:
        f.write('{"version": %s,\n"grid": %s,\n"functions": {\n' % (json.dumps(L.fr_version().decode()), json.dumps(GRID)))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in funcs.items()) + "\n}}\n")


if __name__ == "__main__":
    main()
