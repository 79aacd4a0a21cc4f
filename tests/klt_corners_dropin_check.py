"""Run as its own process by tests/test_gpu_dropin_klt_corners.py: torch first, on the GPU, as the
reference's FeatureFrontend does (frontend.py:3, :66-67), then the ``cfg.klt_corner_replenish`` route
of tests/klt_corners_dropin_scene.py with the feature dicts' tensors on the GPU.  Exit 0 and a final
"OK" line on success, "SKIP: ..." when torch has no GPU here."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

if not torch.cuda.is_available():
    print("SKIP: torch sees no GPU")
    sys.exit(0)
dev = torch.device("cuda")
probe = torch.arange(1024, device=dev, dtype=torch.float32) * 2.0  # torch's HIP runtime is live
torch.cuda.synchronize()

from tests import klt_corners_dropin_scene  # noqa: E402

out = klt_corners_dropin_scene.run(dev)
assert out["corners"] > 0 and out["corners_tracked"] > 0
assert torch.equal((probe / 2.0).cpu(), torch.arange(1024, dtype=torch.float32))  # torch still works
print("OK")
