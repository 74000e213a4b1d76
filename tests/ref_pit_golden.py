"""The reference's PointInTri (render_depth_op.cc:76-122) as the brute-force tests see it: `pit(P[n,8] float64) -> bool[n]`.

Its answers to the exact query stream of every test that uses it are stored under tests/golden/ref_pit/<test>.npz (the
answers, bit-packed, and the sha256 of the queries), so the tests run wherever the suite runs.  Where the reference binary
oracle/_ref/libref_pit.so has been built (oracle/Makefile), the fixture asks the binary and holds the recording to it; with
FR_RECORD_REF_PIT=1 it (re)writes the recording from the binary.  A test whose queries differ from the recorded ones fails:
the recording is only valid for the stream it was made from."""
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

REC_DIR = os.path.join(GOLDEN, "ref_pit")


class _Pit:
    def __init__(self, oracle, name):
        self.path = os.path.join(REC_DIR, re.sub(r"[^A-Za-z0-9_.-]", "_", name) + ".npz")
        self.live = oracle.ref_point_in_tri_batch if oracle.ref_point_in_tri_available() else None
        self.record = self.live is not None and os.environ.get("FR_RECORD_REF_PIT") == "1"
        self.sha = hashlib.sha256()
        self.got = []
        self.want = None
        if not self.record:
            if not os.path.exists(self.path):
                raise AssertionError("no recording of the reference's PointInTri for this test: %s" % self.path)
            with np.load(self.path) as z:
                n = int(z["n"])
                self.want = np.unpackbits(z["answers"])[:n].astype(bool)
                self.want_sha = str(z["sha256"])
        self.pos = 0

    def __call__(self, P):
        P = np.ascontiguousarray(P, dtype=np.float64)
        self.sha.update(P.tobytes())
        if self.want is not None:
            rec = self.want[self.pos:self.pos + P.shape[0]]
            assert rec.shape[0] == P.shape[0], "more PointInTri queries than recorded (%s)" % self.path
        self.pos += P.shape[0]
        if self.live is None:
            return rec.copy()
        out = self.live(P)
        if self.want is not None:
            np.testing.assert_array_equal(out, rec, err_msg="reference binary vs its recording %s" % self.path)
        self.got.append(out)
        return out

    def finish(self):
        if self.record:
            ans = np.concatenate(self.got) if self.got else np.zeros(0, bool)
            os.makedirs(REC_DIR, exist_ok=True)
            np.savez_compressed(self.path, answers=np.packbits(ans), n=np.int64(ans.shape[0]),
                                sha256=np.array(self.sha.hexdigest()))
            return
        assert self.pos == self.want.shape[0] and self.sha.hexdigest() == self.want_sha, \
            "PointInTri queries differ from the recorded stream (%s)" % self.path


@pytest.fixture
def pit(oracle, request):
    p = _Pit(oracle, request.node.name)
    yield p
    p.finish()
