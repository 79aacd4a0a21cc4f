"""Mutual-check matcher calls alone, for a kernel trace (rocprofv3 --kernel-trace --stats, no
counters in the same run): 4000 x 4000 x 128 SIFT-like under the SIFT hint and 2048 x 2048 x 256
SuperPoint-like under the float hint, device-resident, the query side cached.  The forward top-2
sweeps (match_kernel<KS, false>, fsweep_kernel<1, KS, false>) and the reverse top-1 sweeps
(match_kernel<KS, true>, fsweep_kernel<1, KS, true>) carry different names in the trace."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib, matcher  # noqa: E402
from visualodometry_amd._lib import C, check, ptr  # noqa: E402
from visualodometry_amd.synthetic import sift_like_pair, superpoint_like_pair  # noqa: E402

ctx = _lib.context(0)
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
for (d0, d1), kind, tag in ((sift_like_pair(4000, 4000, 7), matcher.DESC_SIFT, 1),
                            (superpoint_like_pair(2048, 2048, 8), matcher.DESC_FLOAT, 2)):
    a, b = _lib.DeviceArray.from_numpy(ctx, d0), _lib.DeviceArray.from_numpy(ctx, d1)
    out = np.empty((d0.shape[0], 2), np.int32)
    cnt = np.zeros(1, np.int32)
    matcher.set_descriptor_kind(kind, ctx)
    for _ in range(calls):
        check(ctx.lib.vo_match_mutual(ctx.handle, C.c_void_p(a.ptr), d0.shape[0], C.c_uint64(tag), C.c_void_p(b.ptr),
                                      d1.shape[0], d0.shape[1], 0.75, _lib.VO_MATCH_DEVICE_PTRS, ptr(out, C.c_int32),
                                      ptr(cnt, C.c_int32)), "vo_match_mutual")
    print(d0.shape, "pairs", int(cnt[0]))
matcher.set_descriptor_kind(matcher.DESC_AUTO, ctx)
