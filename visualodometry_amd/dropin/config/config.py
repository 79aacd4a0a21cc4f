"""``VOConfig`` / ``get_config`` -- same fields, defaults and per-dataset values as
the reference (``src/config/config.py:4-104``), plus the BA knobs of the MI355X
back end (off by default, so behaviour equals the reference).

The per-dataset tuning is kept as data (``_DATASET_OVERRIDES``).  The reference
applies its ``extractor_type == "sift"`` overrides right after building a
default config whose extractor is always ``"superpoint"`` (``config.py:9,51``),
so they never fire (SURVEY.md §5 "Quirk").  ``get_config(dataset)`` reproduces
that exactly; ``get_config(dataset, extractor_type="sift")`` is the documented
extension that selects SIFT and applies those overrides.
"""

from __future__ import annotations

import os
from dataclasses import dataclass


@dataclass
class VOConfig:
    """Configuration of the VO pipeline (field set of reference config.py:4-46)."""

    extractor_type: str = "superpoint"  # superpoint or sift
    global_scale: float = 20.0
    max_keypoints: int = 2048
    device: str = "cuda"
    sift_n_features: int = 2048
    sift_contrast_threshold: float = 0.03
    sift_edge_threshold: float = 1.0
    sift_sigma: float = 1.6
    min_median_flow: float = 20.0
    min_inliers: int = 10
    init_ransac_prob: float = 0.999
    init_ransac_thresh: float = 1.0
    min_depth: float = 0.001
    max_reproj_err: float = 6.0
    pnp_reproj_err: float = 4.0
    kf_min_tracked: int = 80
    turn_thresh: float = 0.01
    move_thresh: float = 0.01
    turn_smoothing: float = 0.7
    trans_smoothing: float = 0.6
    baseline_lr: float = 0.01
    scale_clamp_min: float = 0.5
    scale_clamp_max: float = 3.0
    # ---- MI355X back end (not in the reference) --------------------------------
    ba_enabled: bool = False  # sliding-window BA at keyframe creation
    ba_window: int = 50  # keyframes in the window
    ba_fixed: int = 2  # oldest keyframes held fixed (gauge)
    ba_iters: int = 10  # Gauss-Newton iterations per keyframe
    ba_lambda: float = 1.0  # Levenberg damping: fixed (ba_lm off), or the starting value of the LM schedule
    ba_huber: float = 0.0  # Huber delta of the BA cost in pixels; 0: plain sum of squares
    ba_lm: bool = False  # Levenberg-Marquardt step control on the device (accept / reject, adaptive damping)
    # termination of the LM loop, decided on the device (with ba_lm only); 0: not tested
    ba_lm_ftol: float = 0.0  # stop once an accepted step lowers the cost by at most this fraction
    ba_lm_xtol: float = 0.0  # stop once an accepted step's largest pose-update entry is at most this
    ba_lm_max_rejects: int = 0  # stop after this many rejected steps in a row
    ba_covariance: bool = False  # also read out the pose and landmark covariance of each adjusted window
    # device-side outlier culling: ba_cull_rounds = R > 0 runs R + 1 solves of ba_iters with a cull between them
    ba_cull_rounds: int = 0  # 0: off
    ba_cull_chi2: float = 0.0  # deactivate an observation whose weighted squared error (px^2) exceeds this; 0: not tested
    ba_cull_min_depth: float = 0.0  # deactivate an observation at or below this camera-frame depth
    # marginalisation prior: once the window is full, the oldest keyframe and the landmarks it sees leave as a
    # quadratic cost on the poses that stay, and one fixed pose fewer holds the gauge (2 -> 1 -> 0)
    ba_marginalize: bool = False
    # motion factors: the front end's relative pose between consecutive keyframes, as it stood when the newer one
    # was made, stays in the BA cost as a between factor (it carries the front end's scale)
    ba_motion_factors: bool = False
    ba_motion_sigma_t: float = 0.1  # its translation sigma, map units
    ba_motion_sigma_r: float = 0.02  # its rotation sigma, radians
    sift_on_gpu: bool = True  # SIFT detectAndCompute on the MI355X (frontend.py:27-32,55)
    match_on_gpu: bool = True  # SIFT matching on the MI355X (knn-2 + ratio test)
    match_cross_check: bool = False  # SIFT matching: also require mutual nearest neighbours (one-to-one pairs)
    superpoint_bf_match: bool = False  # SuperPoint: brute-force ratio + cross-check matcher instead of LightGlue
    superpoint_bf_ratio: float = 0.75  # its ratio (frontend.py:104's value; no accuracy measured for SuperPoint)
    triangulate_on_gpu: bool = True  # triangulate_points on the MI355X (DLT + filters)
    pnp_on_gpu: bool = True  # cv2.solvePnPRansac of the tracking step on the MI355X
    init_on_gpu: bool = False  # cv2.findEssentialMat + recoverPose of the initialisation on the MI355X
    map_store_arrays: bool = True  # map_points as an id-indexed array store (MapStore)
    # search by projection: every new keyframe looks for the live map points it did not match, among its
    # unlabelled keypoints inside a window around each point's projection (matcher.match_gated)
    map_reobserve: bool = False
    map_reobserve_radius: float = 15.0  # window radius in pixels (a starting value; nothing measured)
    map_reobserve_ratio: float = 0.8  # ratio test among the keypoints in the window (likewise untuned)
    # largest descriptor distance accepted (a lone keypoint in the window passes the ratio test); None: 300 for
    # SIFT's 0..255 integers, 0.7 for SuperPoint's unit rows (starting values, no accuracy measured)
    map_reobserve_max_dist: float | None = None
    # epipolar search for new landmarks: at every new keyframe, the keypoints of the previous keyframe that
    # the ratio-test match left without a partner are looked for along their epipolar segment in the new one,
    # among its keypoints that have no id and no partner either (matcher.match_segment), and the pairs are
    # triangulated like the keyframe's own.  All values below are untuned starting values; no accuracy claimed.
    map_epipolar_search: bool = False
    map_epipolar_radius: float = 2.0  # distance in pixels a keypoint may lie from the segment
    map_epipolar_ratio: float = 0.8  # ratio test among the keypoints along the segment
    # largest descriptor distance accepted; None: 300 for SIFT's 0..255 integers, 0.7 for SuperPoint's unit rows
    map_epipolar_max_dist: float | None = None
    map_epipolar_min_depth: float = 1.0  # depth range searched, in the previous keyframe's camera ...
    map_epipolar_max_depth: float = 0.0  # ... 0 = up to infinity (the segment ends at the vanishing point)
    # a keypoint whose clipped segment is shorter has no observable depth from this pair: not searched
    map_epipolar_min_length: float = 8.0
    # KLT tracking front end (SIFT extractor only): between two keyframes the keyframe's keypoints are tracked
    # into every frame (visualodometry_amd.klt.track) instead of detecting and matching; the keyframe's
    # descriptors ride along, and a new keyframe is replenished by detection away from the tracked points.
    # All values below are untuned starting values; no accuracy claimed.
    klt_tracking: bool = False
    klt_win_radius: int = 10  # window (2r+1)^2, 21 x 21 as cv2.calcOpticalFlowPyrLK's default
    klt_levels: int = 4  # pyramid levels
    klt_fb_thresh: float = 1.0  # forward-backward check in pixels
    klt_min_tracks: int = 50  # fewer survivors: this frame detects and matches as without the route
    klt_min_distance: float = 8.0  # a replenishing detection keeps this distance from every tracked keypoint
    # replenish a new keyframe with Shi-Tomasi corners (visualodometry_amd.corners.good_features, which reads the
    # keyframe's cached pyramid and keeps away from the tracked points on the device) instead of SIFT detections.
    # The corners carry no SIFT descriptor: the searches that read descriptors of keyframe rows cannot use them, so the
    # switch excludes map_reobserve and map_epipolar_search.  Untuned starting values; no accuracy claimed.
    klt_corner_replenish: bool = False
    klt_corner_quality: float = 0.01  # a corner's response is above this fraction of the strongest one's
    klt_corner_block: int = 3  # block of the gradient sums: 3, 5 or 7
    # give the corners a steered BRIEF descriptor (visualodometry_amd.brief.describe) so that a frame that falls back
    # to detection can find the keyframe's corner rows again: such a frame also receives corners, and match_frames adds
    # the Hamming matches (visualodometry_amd.matcher.match_hamming, cross-checked) between the two sets of corner rows
    # to the SIFT pairs.  Read only under klt_corner_replenish; without it the switch does nothing.  The exclusion of
    # map_reobserve and map_epipolar_search stays.  Untuned starting values; no accuracy claimed.
    klt_corner_describe: bool = False
    klt_brief_ratio: float = 0.8  # ratio test between the two nearest corner rows (untuned starting value)
    klt_brief_max_dist: int = 64  # of 256 bits: the largest distance of a kept pair (untuned starting value)


# dataset -> (overrides always applied, overrides applied when extractor is SIFT)
_DATASET_OVERRIDES = {
    "kitti": (
        dict(min_median_flow=40.0, max_keypoints=2048, max_reproj_err=5.0, pnp_reproj_err=1.0,
             baseline_lr=0.002, turn_smoothing=0.2, trans_smoothing=0.4),
        dict(sift_n_features=4000, sift_contrast_threshold=0.02, sift_edge_threshold=2.0,
             max_reproj_err=5.0, pnp_reproj_err=1.0, turn_smoothing=0.2, trans_smoothing=0.4),
    ),
    "malaga": (
        dict(min_median_flow=30.0, max_keypoints=2048, max_reproj_err=5.0, pnp_reproj_err=2.0,
             baseline_lr=0.003, turn_smoothing=0.5, trans_smoothing=0.3),
        dict(sift_n_features=3000, sift_contrast_threshold=0.01, sift_edge_threshold=2.0,
             max_reproj_err=10.0, min_median_flow=4.0),
    ),
    "parking": (
        dict(min_median_flow=3.0, max_reproj_err=2.0, pnp_reproj_err=1.0),
        dict(sift_n_features=3000, sift_contrast_threshold=0.01, sift_edge_threshold=2.0,
             min_median_flow=4.0),
    ),
    "own": (dict(baseline_lr=0.001, turn_smoothing=0.2, trans_smoothing=0.6), {}),
}


def get_config(dataset: str, extractor_type: str | None = None) -> VOConfig:
    """Config for ``dataset`` (reference config.py:49-104); unknown names get the defaults.

    ``src/main.py`` calls ``get_config(dataset)`` only (``main.py:54``), so two
    environment switches reach the back end without touching it:
    ``VO_AMD_EXTRACTOR=sift`` (as ``extractor_type``), ``VO_AMD_BA=1``
    (``ba_enabled``), ``VO_AMD_SP_BF=1`` (``superpoint_bf_match``), ``VO_AMD_INIT=1``
    (``init_on_gpu``), ``VO_AMD_REOBSERVE=1`` (``map_reobserve``), ``VO_AMD_EPIPOLAR=1``
    (``map_epipolar_search``), ``VO_AMD_KLT=1`` (``klt_tracking``), ``VO_AMD_KLT_CORNERS=1``
    (``klt_corner_replenish``) and ``VO_AMD_KLT_BRIEF=1`` (``klt_corner_describe``).  Unset, the result
    equals the reference's.
    """
    cfg = VOConfig()
    if extractor_type is None:
        extractor_type = os.environ.get("VO_AMD_EXTRACTOR") or None
    if os.environ.get("VO_AMD_BA", "0") not in ("", "0"):
        cfg.ba_enabled = True
    if os.environ.get("VO_AMD_SP_BF", "0") not in ("", "0"):
        cfg.superpoint_bf_match = True
    if os.environ.get("VO_AMD_INIT", "0") not in ("", "0"):
        cfg.init_on_gpu = True
    if os.environ.get("VO_AMD_REOBSERVE", "0") not in ("", "0"):
        cfg.map_reobserve = True
    if os.environ.get("VO_AMD_EPIPOLAR", "0") not in ("", "0"):
        cfg.map_epipolar_search = True
    if os.environ.get("VO_AMD_KLT", "0") not in ("", "0"):
        cfg.klt_tracking = True
    if os.environ.get("VO_AMD_KLT_CORNERS", "0") not in ("", "0"):
        cfg.klt_corner_replenish = True
    if os.environ.get("VO_AMD_KLT_BRIEF", "0") not in ("", "0"):
        cfg.klt_corner_describe = True
    if extractor_type is not None:
        cfg.extractor_type = extractor_type
    base, sift = _DATASET_OVERRIDES.get(dataset, ({}, {}))
    for k, v in base.items():
        setattr(cfg, k, v)
    if cfg.extractor_type == "sift":
        for k, v in sift.items():
            setattr(cfg, k, v)
    return cfg
