"""Child process of tests/test_synth_batch_gpu.py: a process-fresh pipeline.SynthBatches on the small assets; prints the sha256 of
the first batches' tensors.  argv: seed, batch, image size, batches."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from conftest import pkg  # noqa: E402

KEYS = ("im_gray", "params", "depth", "mask", "tri_ind", "light", "alpha")


def digest(batches):
    h = hashlib.sha256()
    for b in batches:
        for k in KEYS:
            h.update(b[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def stream(seed, B, S, **kw):
    dev = torch.device("cuda:0")
    net = pkg("nets.network").FaceRecNet(mesh_data=pkg("utils.synth").make_small_assets(), batch_size=B, im_size=S, device=dev)
    return net, pkg("pipeline").SynthBatches(net, B, seed, focal=1e-3 * S / 200.0, **kw)


def main():
    seed, B, S, n = (int(a) for a in sys.argv[1:5])
    _, st = stream(seed, B, S)
    got = []
    for _ in range(n):
        b = st.next()
        torch.cuda.synchronize()
        got.append({k: b[k].clone() for k in KEYS})
    print("SYNTH_DIGEST " + digest(got))


if __name__ == "__main__":
    main()
