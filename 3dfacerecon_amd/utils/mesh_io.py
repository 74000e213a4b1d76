"""Meshes on the host: the vertex -> triangle adjacency the vertex-normal kernel walks (include/fr_hotpath.h, "fine mesh"), and
writers for one reconstructed face (Wavefront OBJ, ASCII PLY).  numpy only; no reader."""
import numpy as np


def _tri_ids(tri):
    """[3,T] triangle list (float-stored or integer ids) -> int64 [3,T]; a value that is not an integer id becomes -1"""
    t = np.asarray(tri)
    if t.ndim != 2 or t.shape[0] != 3:
        raise ValueError("tri must be [3,T] (got %s)" % (t.shape,))
    if t.dtype.kind == "f":
        ok = np.isfinite(t) & (np.abs(t) < 2.0 ** 31)
        return np.where(ok, np.trunc(np.where(ok, t, 0)), -1).astype(np.int64)   # (the kernels' conversion truncates)
    return t.astype(np.int64)


def vertex_adjacency(tri, nver):
    """The CSR table vertex -> triangles of a [3,T] triangle list over `nver` vertices: (adj_start int32 [nver + 1], adj_tri int32
    [3 T]).  Vertex v's triangles are adj_tri[adj_start[v] : adj_start[v + 1]], in ascending order; a triangle that names a vertex
    twice is listed once for it, and an id outside [0, nver) is listed nowhere.  adj_tri always has 3 T slots (what the kernel's
    contract sizes it by); the slots past adj_start[nver] are padding and hold 0, so adj_start[nver] <= 3 T with equality exactly
    when every triangle names three different vertices of the mesh."""
    ids = _tri_ids(tri)
    nver = int(nver)
    if nver < 0:
        raise ValueError("nver must not be negative")
    T = ids.shape[1]
    t_of = np.tile(np.arange(T, dtype=np.int64), 3)
    v_of = ids.reshape(-1)
    keep = (v_of >= 0) & (v_of < nver)
    pairs = np.unique(np.stack([v_of[keep], t_of[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    counts = np.bincount(pairs[:, 0], minlength=nver)[:nver] if nver else np.zeros((0,), np.int64)
    adj_start = np.zeros(nver + 1, np.int32)
    adj_start[1:] = np.cumsum(counts)
    adj_tri = np.zeros(3 * T, np.int32)
    adj_tri[:len(pairs)] = pairs[:, 1]   # (np.unique sorts by vertex, then by triangle)
    return adj_start, adj_tri


def _face_arrays(vertices, tri, normals, colors, flip_y):
    v = np.asarray(vertices, np.float64)
    if v.ndim != 2 or v.shape[0] != 3:
        raise ValueError("vertices must be one face's [3,N] (got %s)" % (v.shape,))
    N = v.shape[1]
    f = _tri_ids(tri)
    if f.size and (f.min() < 0 or f.max() >= N):
        raise ValueError("tri names a vertex outside [0, %d)" % N)
    out = {"v": v.T.copy(), "f": f.T.copy(), "n": None, "c": None}
    for key, a in (("n", normals), ("c", colors)):
        if a is not None:
            a = np.asarray(a, np.float64)
            if a.shape != (3, N):
                raise ValueError("%s must be [3,%d] (got %s)" % ("normals" if key == "n" else "colors", N, a.shape))
            out[key] = a.T.copy()
    if flip_y is not None:
        # the decode stores y as (im_size - y) - 1, a mirror: undo it, and reverse the winding it reversed
        out["v"][:, 1] = (float(flip_y) - out["v"][:, 1]) - 1.0
        out["f"] = out["f"][:, ::-1].copy()
        if out["n"] is not None:
            out["n"][:, 1] = -out["n"][:, 1]
    return out


def write_obj(path, vertices, tri, normals=None, colors=None, flip_y=None):
    """One face as a Wavefront OBJ: `vertices` [3,N], `tri` [3,T] 0-based ids (float-stored or integer), written 1-based.
    normals [3,N]: `vn` lines and `f a//a b//b c//c`.  colors [3,N] in [0, 1]: appended to the `v` lines (the common extension).
    flip_y=im_size: y is written as (im_size - y) - 1 -- the decode's flip undone, so the file is upright -- the winding of every
    face is reversed with it and the normals' y negated, so the faces and normals keep pointing out."""
    a = _face_arrays(vertices, tri, normals, colors, flip_y)
    with open(path, "w") as fh:
        fh.write("# %d vertices, %d faces\n" % (len(a["v"]), len(a["f"])))
        for i, p in enumerate(a["v"]):
            if a["c"] is None:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
            else:
                fh.write("v %.9g %.9g %.9g %.6g %.6g %.6g\n" % (tuple(p) + tuple(a["c"][i])))
        if a["n"] is not None:
            for n in a["n"]:
                fh.write("vn %.9g %.9g %.9g\n" % tuple(n))
        for t in a["f"] + 1:
            if a["n"] is None:
                fh.write("f %d %d %d\n" % tuple(t))
            else:
                fh.write("f %d//%d %d//%d %d//%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2]))


def write_ply(path, vertices, tri, normals=None, colors=None, flip_y=None):
    """One face as an ASCII PLY, arguments as write_obj; faces are 0-based, colors become uchar red / green / blue."""
    a = _face_arrays(vertices, tri, normals, colors, flip_y)
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex %d\n" % len(a["v"]))
        fh.write("property float x\nproperty float y\nproperty float z\n")
        if a["n"] is not None:
            fh.write("property float nx\nproperty float ny\nproperty float nz\n")
        if a["c"] is not None:
            fh.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        fh.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(a["f"]))
        for i, p in enumerate(a["v"]):
            line = "%.9g %.9g %.9g" % tuple(p)
            if a["n"] is not None:
                line += " %.9g %.9g %.9g" % tuple(a["n"][i])
            if a["c"] is not None:
                line += " %d %d %d" % tuple(int(round(min(max(c, 0.0), 1.0) * 255)) for c in a["c"][i])
            fh.write(line + "\n")
        for t in a["f"]:
            fh.write("3 %d %d %d\n" % tuple(t))
