"""Run as its own process by tests/test_gpu_dropin_superpoint.py: torch first, on the GPU, as the
reference's FeatureFrontend does (frontend.py:3, :66-67), then the patched match_frames on the
feature dicts' (1, N, 256) CUDA tensors with the SuperPoint brute-force switch on.  Exit 0 and a
final "OK" line on success, "SKIP: ..." when torch has no GPU here."""

import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

if not torch.cuda.is_available():
    print("SKIP: torch sees no GPU")
    sys.exit(0)
dev = torch.device("cuda")
probe = torch.arange(1024, device=dev, dtype=torch.float32) * 2.0  # torch's HIP runtime is live
torch.cuda.synchronize()

from tests import mutual_ref  # noqa: E402
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.dropin import hooks  # noqa: E402

d0, d1 = mutual_ref.superpoint_near_duplicates(700, 900, 3, 150)
ref, n_forward = mutual_ref.mutual(d0, d1, 0.75, "c")
assert mutual_ref.informative(ref, n_forward)
frontend = SimpleNamespace(conf=SimpleNamespace(extractor_type="superpoint", superpoint_bf_match=True,
                                                superpoint_bf_ratio=0.75))
match_frames = hooks._wrap_match_frames(lambda self, a, b: "original")
feats0 = {"descriptors": torch.from_numpy(d0)[None].to(dev)}
feats1 = {"descriptors": torch.from_numpy(d1)[None].to(dev)}
got = match_frames(frontend, feats0, feats1)
assert got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2
assert np.array_equal(got, ref), "superpoint brute-force route mismatch vs the reference composition"
# the keyframe side stays cached across frames (the same GPU tensor) for both roles it plays
d2 = np.ascontiguousarray(d1[::-1][:650])
ref2, nf2 = mutual_ref.mutual(d0, d2, 0.75, "c")
assert mutual_ref.informative(ref2, nf2)
feats2 = {"descriptors": torch.from_numpy(d2)[None].to(dev)}
assert np.array_equal(match_frames(frontend, feats0, feats2), ref2), "cached keyframe mismatch"
feats0["descriptors"][0, 3] = feats0["descriptors"][0, 7]  # in place on the GPU: a new version
m0 = feats0["descriptors"][0].cpu().numpy()
assert np.array_equal(match_frames(frontend, feats0, feats1), mutual_ref.mutual(m0, d1, 0.75, "c")[0]), \
    "modified keyframe mismatch"
empty = {"descriptors": torch.zeros((1, 0, 256), device=dev)}
one = {"descriptors": feats1["descriptors"][:, :1].contiguous()}
for a, b in ((empty, feats1), (feats0, empty), (feats0, one)):
    r = match_frames(frontend, a, b)
    assert r.shape == (0, 2) and r.dtype == np.int64
frontend.conf.superpoint_bf_match = False
assert match_frames(frontend, feats0, feats1) == "original"
print("device tensors read in place:", not getattr(_lib.context(), "_foreign_tensors", False))
assert torch.equal((probe / 2.0).cpu(), torch.arange(1024, dtype=torch.float32))
print("OK")
