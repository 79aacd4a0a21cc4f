"""Runtime hooks that put the MI355X matcher and BA under the reference's VO loop.

Nothing of the reference is copied: :func:`install` patches methods of the
reference's own classes and names of its modules once they are imported (cv2 etc.
are the caller's environment):

* ``FeatureFrontend.__init__`` (reference ``src/modules/frontend.py:10-34``): with the SIFT
  extractor and ``cfg.sift_on_gpu`` (default on), ``self.extractor`` becomes
  :func:`visualodometry_amd.sift.SIFT_create` with the same nfeatures / contrast / edge /
  sigma, so ``process_image`` (``:51-75``) runs detectAndCompute on the MI355X.
* ``FeatureFrontend.match_frames`` (reference ``src/modules/frontend.py:78-113``),
  SIFT branch -> :func:`visualodometry_amd.matcher.match_knn2_ratio`.  The
  LightGlue branch (``:80-84``) is left to the original method.
* ``triangulate_points`` (``src/modules/frontend.py:115-148``, imported by name into
  ``vo.py``) -> :func:`visualodometry_amd.triangulate.triangulate_points` in both
  modules (``cfg.triangulate_on_gpu``, default on).
* ``VisualOdometry._create_keyframe`` (``src/modules/vo.py:252-288``) is wrapped:
  the original triangulates and rotates the keyframe, then
  :class:`KeyframeWindow` records the new keyframe and, if ``cfg.ba_enabled``,
  runs :class:`~visualodometry_amd.ba.SlidingWindowBA` on the last
  ``cfg.ba_window`` keyframes and writes poses and map points back
  (SURVEY.md §8a row a11).  With ``cfg.ba_motion_factors`` the window also keeps the front end's
  relative pose between consecutive keyframes (the motion ``vo.py:152-204`` produced) as between
  factors of that BA, which otherwise overwrites it.  With ``cfg.map_reobserve`` (off by default)
  the new keyframe first looks for the live map points it did not match (:func:`reobserve_map`:
  search by projection, :func:`visualodometry_amd.matcher.match_gated`), so a landmark that missed
  one keyframe-to-keyframe match gets its id back instead of a duplicate beside it.  With
  ``cfg.map_epipolar_search`` (off by default) the keypoints that match left without a partner are
  then looked for along their epipolar segments (:func:`epipolar_search`,
  :func:`visualodometry_amd.matcher.match_segment`) and the pairs triangulated into new landmarks.
* With ``cfg.klt_tracking`` (off by default, SIFT extractor only) ``process_image`` tracks the
  keyframe's keypoints into the frame (:func:`klt_process_image`,
  :func:`visualodometry_amd.klt.track`) instead of detecting, ``match_frames`` returns the pairs a
  tracked frame brings (:func:`klt_pairs`), and a new keyframe is replenished by detection away
  from its tracked keypoints (:func:`klt_replenish`).  The settings are read once, when the
  frontend is constructed; a frontend without the route reads no ``klt_*`` setting on the frame path.
  With ``cfg.klt_corner_replenish`` (off by default) the replenishment takes Shi-Tomasi corners
  (:func:`visualodometry_amd.corners.good_features`) instead of SIFT detections; their rows have no
  descriptor (a per-row flag says so) and a detected frame is matched against the others only.
  With ``cfg.klt_corner_describe`` on top (off by default) the corners get steered BRIEF rows
  (:func:`visualodometry_amd.brief.describe`), a frame that falls back to detection receives
  described corners too, and ``match_frames`` adds the cross-checked Hamming matches between the
  two sets of corner rows (:func:`visualodometry_amd.matcher.match_hamming`) to the SIFT pairs.

The reference keeps only the current keyframe's observation of a freshly
triangulated point (``vo.py:277-284``); the window also records the previous
keyframe's observation of it (the other ray of the triangulation), which is
what makes a two-keyframe landmark constrain BA at all.
"""

from __future__ import annotations

import itertools
import weakref
from collections import deque
from dataclasses import dataclass, field

import numpy as np

from ..ba import BAResult, BAWindow, PoseFactor, SlidingWindowBA
from ..mapstore import MAX_POINTS, LandmarkDescriptors, MapStore


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _keypoints(feats: dict) -> np.ndarray:
    kp = _np(feats["keypoints"])
    return kp[0] if kp.ndim == 3 else kp


@dataclass
class KeyframeRecord:
    T_wc: np.ndarray  # (4,4) f64 camera -> world (the reference's pose storage, vo.py:19)
    uv: np.ndarray  # (N,2) f32 keypoints
    ids: np.ndarray  # (N,) int landmark id per keypoint, -1 if none
    extra_uv: list = field(default_factory=list)  # observations added after the keyframe was made
    extra_ids: list = field(default_factory=list)
    # motion factors (cfg.ba_motion_factors): the front end's T_cw(previous keyframe) T_cw(this)^-1 as
    # the two stood when this keyframe was added, before BA; None: not recorded
    motion: np.ndarray | None = None


class KeyframeWindow:
    """The last ``size`` keyframes and their landmark observations.

    ``max_track`` caps the observations of one landmark to its most recent
    keyframes: the BA planner handles at most 10 free cameras per landmark
    (DESIGN.md §BA layout).

    ``motion_factors`` (``cfg.ba_motion_factors``, off by default): every keyframe records the front
    end's relative pose to the one before it, and ``build`` emits one between factor per consecutive
    pair still in the window, with information ``diag(1/sigma_t^2 x3, 1/sigma_r^2 x3)``.  The record
    lives on the newer keyframe of a pair, and a pair is emitted only while both are in the window:
    one whose older keyframe left went into the prior (``cfg.ba_marginalize``) or was dropped.
    """

    def __init__(self, size: int = 50, n_fixed: int = 2, max_track: int = 10, motion_factors: bool = False,
                 motion_sigma_t: float = 0.1, motion_sigma_r: float = 0.02):
        self.motion_factors = bool(motion_factors)
        if self.motion_factors and not (motion_sigma_t > 0 and motion_sigma_r > 0):
            raise ValueError("ba_motion_sigma_t and ba_motion_sigma_r must be > 0")
        self.motion_info = np.diag([1.0 / motion_sigma_t**2] * 3 + [1.0 / motion_sigma_r**2] * 3) \
            if self.motion_factors else None
        self.size = int(size)
        self.n_fixed = int(n_fixed)
        self.max_track = int(max_track)
        self.frames: deque[KeyframeRecord] = deque(maxlen=self.size)
        # marginalisation (cfg.ba_marginalize, slide()): the prior what left the window handed to
        # the poses that stay, the landmark ids it absorbed, and the fixed poses of the next window
        self.prior = None
        self.marginalised: set = set()
        self.cur_fixed = self.n_fixed

    def reset(self) -> None:
        self.frames.clear()
        self.clear_prior()
        self.marginalised.clear()

    def clear_prior(self) -> None:
        """Back to a window without a prior: the configured fixed poses hold the gauge again.  The
        absorbed landmarks stay out of the window (their information went with the prior)."""
        self.prior = None
        self.cur_fixed = self.n_fixed

    def full(self) -> bool:
        return len(self.frames) == self.size

    def slide(self, prior, absorbed_ids) -> None:
        """The oldest keyframe leaves now (the next ``add`` would drop it anyway): ``prior`` is what it
        and the landmarks ``absorbed_ids`` leave on the poses that stay, which one fixed pose fewer
        holds from here on.  Those landmarks stay in the map for PnP and leave ``observations``."""
        self.frames.popleft()
        self.prior = prior
        self.marginalised.update(int(i) for i in np.asarray(absorbed_ids).reshape(-1))
        self.cur_fixed = max(0, self.cur_fixed - 1)
        # ids no keyframe of the window observes any more have nothing left to be kept out of
        # (ids are never reused), so the set stays the size of what the window can see
        seen = [a for fr in self.frames for a in [fr.ids] + fr.extra_ids]
        if seen:
            self.marginalised.intersection_update(np.unique(np.concatenate(seen)).tolist())
        else:
            self.marginalised.clear()

    def add(self, T_wc, uv, ids, prev_uv=None, prev_ids=None) -> None:
        """Append a keyframe; ``prev_uv/prev_ids`` are new observations of the previous keyframe."""
        if prev_ids is not None and len(prev_ids) and self.frames:
            last = self.frames[-1]
            last.extra_uv.append(np.asarray(prev_uv, np.float32).reshape(-1, 2))
            last.extra_ids.append(np.asarray(prev_ids, np.int64))
        T_wc = np.array(T_wc, np.float64)
        motion = None
        if self.motion_factors and self.frames:  # T_cw(prev) T_cw(new)^-1 = T_wc(prev)^-1 T_wc(new)
            motion = np.linalg.inv(self.frames[-1].T_wc) @ T_wc
        self.frames.append(KeyframeRecord(T_wc, np.asarray(uv, np.float32).reshape(-1, 2), np.array(ids, np.int64),
                                          motion=motion))

    def factors(self):
        """The motion factors of the consecutive pairs in the window (``None`` with the switch off or
        nothing recorded): between window cameras ``k - 1`` and ``k``, from keyframe ``k``'s record."""
        if not self.motion_factors:
            return None
        out = [PoseFactor(k - 1, k, fr.motion, self.motion_info)
               for k, fr in enumerate(self.frames) if k > 0 and fr.motion is not None]
        return out or None

    def observations(self, map_points: dict):
        """-> (obs_kf, obs_uv, obs_id) of every window observation of a landmark still in the map."""
        kf, uv, pid = [], [], []
        for k, fr in enumerate(self.frames):
            us = [fr.uv] + fr.extra_uv
            ids = [fr.ids] + fr.extra_ids
            u = np.concatenate(us)
            i = np.concatenate(ids)
            if isinstance(map_points, MapStore):
                keep = map_points.contains(i)
            else:
                keep = (i >= 0) & np.fromiter((int(x) in map_points for x in i), bool, i.size)
            if self.marginalised:
                keep = keep & ~np.isin(i, np.fromiter(self.marginalised, np.int64, len(self.marginalised)))
            kf.append(np.full(int(keep.sum()), k, np.int32))
            uv.append(u[keep])
            pid.append(i[keep])
        if not kf:
            return np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros(0, np.int64)
        return np.concatenate(kf), np.concatenate(uv), np.concatenate(pid)

    def build(self, map_points: dict):
        """-> (BAWindow, landmark ids) or (None, None) if the window has nothing to adjust."""
        if len(self.frames) <= self.cur_fixed:
            return None, None
        kf, uv, pid = self.observations(map_points)
        if pid.size == 0:
            return None, None
        # group by landmark, newest keyframe first; rank the distinct keyframes of each landmark
        order = np.lexsort((-kf, pid))
        kf, uv, pid = kf[order], uv[order], pid[order]
        new_pt = np.r_[True, pid[1:] != pid[:-1]]
        new_kf = new_pt | np.r_[True, kf[1:] != kf[:-1]]
        grp = np.cumsum(new_pt) - 1
        c = np.cumsum(new_kf)
        kf_rank = c - c[new_pt][grp]  # 0 = newest keyframe of this landmark
        keep = kf_rank < self.max_track
        kf, uv, pid, grp, new_kf = kf[keep], uv[keep], pid[keep], grp[keep], new_kf[keep]
        ids = pid[new_pt[keep]]  # the newest keyframe of every landmark is always kept
        n_kf = np.bincount(grp, weights=new_kf, minlength=ids.size)
        inv = grp
        good = n_kf >= 2  # a landmark needs two distinct keyframes to be constrained
        if not good.any():
            return None, None
        sel = good[inv]
        kf, uv, inv = kf[sel], uv[sel], inv[sel]
        remap = -np.ones(ids.size, np.int64)
        remap[good] = np.arange(int(good.sum()))
        lm_ids = ids[good]
        if isinstance(map_points, MapStore):
            points = map_points.gather(lm_ids).astype(np.float64)
        else:
            points = np.stack([np.asarray(map_points[int(i)], np.float64).reshape(3) for i in lm_ids])
        poses_cw = np.stack([np.linalg.inv(fr.T_wc) for fr in self.frames])
        w = BAWindow(poses_cw=poses_cw, points=points, obs_uv=uv.astype(np.float32), obs_cam=kf.astype(np.int32),
                     obs_pt=remap[inv].astype(np.int32), n_fixed=self.cur_fixed)
        if self.prior is not None and self.prior.n_poses <= len(self.frames) - self.cur_fixed:
            w.prior = self.prior
        w.factors = self.factors()
        return w, lm_ids

    def write_back(self, res: BAResult, lm_ids, map_points: dict, obs_pt=None) -> None:
        """``obs_pt``: the window's landmark per observation, needed only under culling
        (``res.obs_active``)."""
        for fr, P in zip(self.frames, res.poses_cw):
            fr.T_wc = np.linalg.inv(P)
        lm_ids, points = np.asarray(lm_ids), np.asarray(res.points)
        if res.obs_active is not None and obs_pt is not None:
            # culling: a landmark all of whose observations were culled was held by nothing
            live = np.bincount(np.asarray(obs_pt)[res.obs_active], minlength=lm_ids.size) > 0
            lm_ids, points = lm_ids[live], points[live]
        if isinstance(map_points, MapStore):
            map_points.scatter(lm_ids, points)
            return
        for i, X in zip(lm_ids, points):
            old = map_points[int(i)]
            map_points[int(i)] = np.asarray(X, dtype=np.asarray(old).dtype).reshape(np.shape(old))


def _wrap_create_keyframe(orig):
    def _create_keyframe(self, curr_feats, curr_ids, ref_indices, curr_indices):
        cfg = self.cfg
        win = getattr(self, "_vo_amd_window", None)
        if win is None:
            win = KeyframeWindow(getattr(cfg, "ba_window", 50), getattr(cfg, "ba_fixed", 2),
                                 motion_factors=getattr(cfg, "ba_motion_factors", False),
                                 motion_sigma_t=getattr(cfg, "ba_motion_sigma_t", 0.1),
                                 motion_sigma_r=getattr(cfg, "ba_motion_sigma_r", 0.02))
            self._vo_amd_window = win
        prev = self.keyframe
        if prev is not None and not win.frames:  # the window starts at the keyframe before the first
            win.add(prev["T_wc"], _keypoints(prev["feats"]), prev["ids"])
        first_new = self.next_pt_id
        ref_indices = np.asarray(ref_indices)
        curr_indices = np.asarray(curr_indices)
        no_id = curr_ids[curr_indices] == -1
        orig(self, curr_feats, curr_ids, ref_indices, curr_indices)
        if getattr(cfg, "map_reobserve", False):  # (off: no attribute, no call, no array touched)
            reobserve_map(self, curr_feats, curr_ids, first_new)
        found = None
        if getattr(cfg, "map_epipolar_search", False) and prev is not None:  # (off: as map_reobserve)
            found = epipolar_search(self, prev, curr_feats, curr_ids, ref_indices, curr_indices)
        # the previous keyframe saw every newly triangulated point (vo.py:265-284)
        cand = curr_indices[no_id]
        new_ids = curr_ids[cand]
        # a current keypoint matched by several reference keypoints (no cross-check,
        # frontend.py:34) had its id overwritten in the loop: its other ray is ambiguous
        uniq, cnt = np.unique(cand, return_counts=True)
        is_new = (new_ids >= first_new) & np.isin(cand, uniq[cnt == 1])
        prev_uv = _keypoints(prev["feats"])[ref_indices[no_id][is_new]] if prev is not None else None
        prev_ids = new_ids[is_new]
        if found is not None and len(found[1]):  # the epipolar search's landmarks: their other ray too
            prev_uv = np.concatenate([np.asarray(prev_uv, np.float32).reshape(-1, 2), found[0]])
            prev_ids = np.concatenate([prev_ids, found[1]])
        win.add(self.T_wc, _keypoints(curr_feats), curr_ids, prev_uv, prev_ids)
        if getattr(cfg, "ba_enabled", False):
            self._vo_amd_last_ba = run_window_ba(self, win)
        fe = getattr(self, "frontend", None)
        st = getattr(fe, "_vo_amd_klt", None)  # (off: not set; no klt_* setting is read, no call made)
        if st is not None:
            klt_replenish(self, st, lambda image: _detect_as_today(fe, image))

    _create_keyframe._vo_amd_wrapped = orig
    return _create_keyframe


def _descriptors(feats: dict):
    d = feats["descriptors"]
    return d[0] if getattr(d, "ndim", 2) == 3 else d


def _rows(a, idx: np.ndarray):
    """Rows ``idx`` of a numpy array or torch tensor (a tensor stays on its device)."""
    if hasattr(a, "detach"):
        import torch

        return a[torch.as_tensor(idx, dtype=torch.long, device=a.device)]
    return np.asarray(a)[idx]


def _image_size(feats: dict, K) -> tuple:
    """(width, height): the feature dict's ``image_size`` (frontend.py:74), else twice the principal point."""
    size = feats.get("image_size")
    if size is not None:
        w, h = _np(size).reshape(-1)[:2]
        return int(w), int(h)
    return int(round(2.0 * K[0, 2])), int(round(2.0 * K[1, 2]))


def reobserve_map(vo, curr_feats, curr_ids, first_new: int) -> int:
    """``cfg.map_reobserve``: after the keyframe's own association, record the descriptors of the
    landmarks it created (ids ``>= first_new``), then offer every live map point that is not among
    ``curr_ids``, has a stored descriptor and projects into the image to the keypoints that still
    have no id, within ``cfg.map_reobserve_radius`` pixels of its projection under ``vo.T_wc``.
    Matched ids are written into ``curr_ids`` in place (the array the keyframe keeps as ``ids``),
    one-to-one.  Returns how many."""
    from .. import matcher

    cfg = vo.cfg
    store = getattr(vo, "_vo_amd_lm_desc", None)
    if store is None:
        store = vo._vo_amd_lm_desc = LandmarkDescriptors()
    des = _descriptors(curr_feats)
    new = np.flatnonzero(curr_ids >= first_new)
    if new.size:
        store.put(curr_ids[new], _np(_rows(des, new)))
    mp = vo.map_points
    if isinstance(mp, MapStore):
        ids, xyz = mp.arrays()
    else:
        ids = np.array(sorted(mp), np.int64)
        xyz = np.array([np.asarray(mp[int(i)], np.float64).reshape(3) for i in ids]).reshape(-1, 3)
    free = np.flatnonzero(curr_ids == -1)
    offer = ~np.isin(ids, curr_ids[curr_ids >= 0]) & store.contains(ids)
    if not offer.any() or free.size == 0:
        return 0
    ids, xyz = ids[offer], xyz[offer]
    size = _image_size(curr_feats, vo.K)
    pred, valid = matcher.project_points(xyz, np.linalg.inv(vo.T_wc), vo.K, size, getattr(cfg, "min_depth", 0.0))
    if not valid.any():
        return 0
    ids, pred = ids[valid], pred[valid]  # (a point outside the frame would only be an inactive query)
    max_dist = getattr(cfg, "map_reobserve_max_dist", None)
    if max_dist is None:
        max_dist = 0.7 if getattr(cfg, "extractor_type", "sift") == "superpoint" else 300.0
    kp = curr_feats["keypoints"]
    kp = kp[0] if getattr(kp, "ndim", 2) == 3 else kp
    pairs = matcher.match_gated(store.gather(ids), pred, float(getattr(cfg, "map_reobserve_radius", 15.0)),
                                _rows(des, free), _rows(kp, free),
                                ratio=float(getattr(cfg, "map_reobserve_ratio", 0.8)), max_dist=float(max_dist),
                                unique=True, image_size=size)
    curr_ids[free[pairs[:, 1]]] = ids[pairs[:, 0]]
    return len(pairs)


def epipolar_search(vo, prev, curr_feats, curr_ids, ref_indices, curr_indices):
    """``cfg.map_epipolar_search``: new landmarks from the keypoints the ratio-test match dropped.

    Queries are the previous keyframe's keypoints that have no id and took no part in the match
    (not in ``ref_indices``); train rows are the new frame's keypoints without an id that took no
    part either (not in ``curr_indices``), so the landmarks the keyframe's own association made or
    carried keep their keypoints, and the ids made here never sit on a matched keypoint.  Both
    poses are known, so each query is looked for only along its epipolar segment in the new frame
    (:func:`visualodometry_amd.matcher.epipolar_segments` over the configured depth range, then
    :func:`visualodometry_amd.matcher.match_segment`, one-to-one).  The pairs are triangulated
    and filtered as the keyframe's own (``triangulate_points``: ``cfg.min_depth``,
    ``cfg.max_reproj_err``); each kept point takes ``next_pt_id`` in ascending query order, goes
    into ``map_points`` as float32 and into ``curr_ids``, and with ``cfg.map_reobserve`` its
    descriptor into the landmark descriptor store.  ``_prune_map`` runs once more.

    Returns ``(uv (M, 2) float32, ids (M,) int64)``: the new landmarks' observations in the
    previous keyframe, for the window."""
    from .. import matcher, triangulate

    cfg = vo.cfg
    none = np.zeros((0, 2), np.float32), np.zeros(0, np.int64)
    prev_ids = np.asarray(prev["ids"])
    q_mask = prev_ids == -1
    q_mask[np.asarray(ref_indices, np.int64)] = False
    t_mask = curr_ids == -1
    t_mask[np.asarray(curr_indices, np.int64)] = False
    q, free = np.flatnonzero(q_mask), np.flatnonzero(t_mask)
    if q.size == 0 or free.size == 0:
        return none
    kp0, kp1 = _keypoints(prev["feats"]), _keypoints(curr_feats)
    size = _image_size(curr_feats, vo.K)
    T_cw_prev, T_cw_cur = np.linalg.inv(prev["T_wc"]), np.linalg.inv(vo.T_wc)
    z_max = float(getattr(cfg, "map_epipolar_max_depth", 0.0))
    seg, valid = matcher.epipolar_segments(kp0[q], T_cw_prev, T_cw_cur, vo.K, size,
                                           float(getattr(cfg, "map_epipolar_min_depth", 1.0)),
                                           z_max if z_max > 0 else np.inf,
                                           float(getattr(cfg, "map_epipolar_min_length", 8.0)))
    if not valid.any():
        return none
    q, seg = q[valid], seg[valid]  # (a keypoint without a segment would only be an inactive query)
    max_dist = getattr(cfg, "map_epipolar_max_dist", None)
    if max_dist is None:
        max_dist = 0.7 if getattr(cfg, "extractor_type", "sift") == "superpoint" else 300.0
    des0, des1 = _descriptors(prev["feats"]), _descriptors(curr_feats)
    kp = curr_feats["keypoints"]
    kp = kp[0] if getattr(kp, "ndim", 2) == 3 else kp
    pairs = matcher.match_segment(_np(_rows(des0, q)), seg, float(getattr(cfg, "map_epipolar_radius", 2.0)),
                                  _rows(des1, free), _rows(kp, free),
                                  ratio=float(getattr(cfg, "map_epipolar_ratio", 0.8)), max_dist=float(max_dist),
                                  unique=True, image_size=size)
    if len(pairs) == 0:
        return none
    qi, ci = q[pairs[:, 0]], free[pairs[:, 1]]
    pts3d, keep = triangulate.triangulate_points(T_cw_prev, T_cw_cur, kp0[qi], kp1[ci], vo.K, cfg)
    keep = np.asarray(keep, bool)
    if not keep.any():
        return none
    qi, ci = qi[keep], ci[keep]
    ids = np.arange(vo.next_pt_id, vo.next_pt_id + len(qi), dtype=np.int64)
    for pid, X in zip(ids, np.asarray(pts3d, np.float32).reshape(-1, 3)):
        vo.map_points[int(pid)] = X
    curr_ids[ci] = ids
    vo.next_pt_id += len(ids)
    store = getattr(vo, "_vo_amd_lm_desc", None)
    if getattr(cfg, "map_reobserve", False) and store is not None:
        store.put(ids, _np(_rows(des1, ci)))
    prune = getattr(vo, "_prune_map", None)
    if prune is not None:
        prune()
    return np.asarray(kp0[qi], np.float32).reshape(-1, 2), ids


# ---- cfg.klt_tracking: the KLT tracking front end --------------------------------------------
# Private keys of a feature dict under the route: the frame's grey image and the tag its device
# pyramid is cached under, and, on a dict tracked from a keyframe, that keyframe's dict and the
# keyframe row of each of its rows.
_KLT_IMAGE, _KLT_TAG, _KLT_SRC, _KLT_SRC_IDX = "_vo_amd_klt_image", "_vo_amd_klt_tag", "_vo_amd_klt_src", \
    "_vo_amd_klt_src_idx"
_KLT_HAS_DESC = "_vo_amd_klt_has_desc"  # cfg.klt_corner_replenish: (N,) bool, which rows carry a real descriptor
_KLT_BRIEF = "_vo_amd_klt_brief"  # cfg.klt_corner_describe: (N, 8) uint32 BRIEF rows (zeros for rows with a descriptor)
_klt_tags = itertools.count(1 << 40)  # pyramid-cache tags of the frames seen (one per image, never reused)


class KltTracker:
    """State of the ``cfg.klt_tracking`` route on a ``FeatureFrontend``: the settings (read once,
    at construction), the ``VisualOdometry`` that owns the frontend, and per keyframe dict the
    keyframe rows still alive with their positions in the previous frame.  A point once lost
    stays lost until the next keyframe."""

    def __init__(self, config):
        self.win_radius = int(getattr(config, "klt_win_radius", 10))
        self.levels = int(getattr(config, "klt_levels", 4))
        self.fb_thresh = float(getattr(config, "klt_fb_thresh", 1.0))
        self.min_tracks = int(getattr(config, "klt_min_tracks", 50))
        self.min_distance = float(getattr(config, "klt_min_distance", 8.0))
        self.max_rows = int(getattr(config, "sift_n_features", 0) or 0)
        self.corners = bool(getattr(config, "klt_corner_replenish", False))
        self.describe = False
        if self.corners:  # (off: neither setting is read)
            self.corner_quality = float(getattr(config, "klt_corner_quality", 0.01))
            self.corner_block = int(getattr(config, "klt_corner_block", 3))
            self.describe = bool(getattr(config, "klt_corner_describe", False))
            if self.describe:  # (off: neither setting is read)
                self.brief_ratio = float(getattr(config, "klt_brief_ratio", 0.8))
                self.brief_max_dist = int(getattr(config, "klt_brief_max_dist", 64))
            for other in ("map_reobserve", "map_epipolar_search"):
                if getattr(config, other, False):
                    raise ValueError(f"klt_corner_replenish cannot be combined with {other}: that search reads "
                                     "descriptors of keyframe rows, and a corner's row has none")
        self.owner = None  # weakref to the VisualOdometry (set by its wrapped __init__)
        self.reset()

    def reset(self) -> None:
        self.src = None    # the keyframe dict the state below belongs to
        self.alive = None  # (M,) int64 keyframe rows still tracked
        self.last = None   # (M, 2) float32 their positions in the previous frame: the next guess
        self.kp0 = None    # (N, 2) float32 the keyframe's keypoints

    def keyframe(self):
        vo = self.owner() if self.owner is not None else None
        return getattr(vo, "keyframe", None) if vo is not None else None


def _like(a, ref):
    """The numpy array ``a`` as ``ref``'s kind: a tensor on ``ref``'s device, or numpy."""
    if hasattr(ref, "detach"):
        import torch

        return torch.from_numpy(np.ascontiguousarray(a)).to(ref.device)
    return a


def _batched(a, ref):
    return a[None] if getattr(ref, "ndim", 2) == 3 else a


def klt_process_image(st: KltTracker, img, detect):
    """``process_image`` under ``cfg.klt_tracking``.  Without a keyframe that carries its image,
    ``detect()`` (the frame path without the route) and the image attached; otherwise the
    keyframe's live keypoints tracked into ``img``: the survivors' positions as ``keypoints``,
    their keyframe descriptors as ``descriptors``.  Fewer than ``klt_min_tracks`` survivors:
    ``detect()`` for this frame."""
    from .. import klt

    if np.ndim(img) != 2 or getattr(img, "dtype", None) != np.uint8:
        return detect()  # the route tracks grey uint8 frames only
    tag = next(_klt_tags)

    def detected():
        feats = detect()
        if isinstance(feats, dict):
            feats[_KLT_IMAGE], feats[_KLT_TAG] = img, tag
        return feats

    kf = st.keyframe()
    src = kf.get("feats") if isinstance(kf, dict) else None
    if not isinstance(src, dict) or src.get(_KLT_IMAGE) is None or src[_KLT_IMAGE].shape != img.shape:
        return detected()
    kp_ref = src["keypoints"]
    if st.src is not src:  # a new keyframe: all of its rows are alive again
        st.src = src
        st.last = np.ascontiguousarray(_keypoints(src), np.float32).reshape(-1, 2)
        st.alive = np.arange(len(st.last), dtype=np.int64)
        st.kp0 = st.last.copy()
    if st.alive.size < st.min_tracks:
        return klt_describe_fallback(st, detected(), img, tag) if st.describe else detected()
    p1, status, _ = klt.track(src[_KLT_IMAGE], img, st.kp0[st.alive], guess=st.last, win_radius=st.win_radius,
                              levels=st.levels, fb_thresh=st.fb_thresh if st.fb_thresh > 0 else None,
                              tags=(src[_KLT_TAG], tag))
    ok = status == 0
    st.alive, st.last = st.alive[ok], np.ascontiguousarray(p1[ok])
    if st.alive.size < st.min_tracks:
        return klt_describe_fallback(st, detected(), img, tag) if st.describe else detected()
    feats = {
        "keypoints": _batched(_like(st.last, kp_ref), kp_ref),
        "descriptors": _batched(_rows(_descriptors(src), st.alive), src["descriptors"]),
        _KLT_IMAGE: img, _KLT_TAG: tag, _KLT_SRC: src, _KLT_SRC_IDX: st.alive,
    }
    if "image_size" in src:
        feats["image_size"] = src["image_size"]
    if _KLT_HAS_DESC in src:  # cfg.klt_corner_replenish: the flag follows its descriptor row
        feats[_KLT_HAS_DESC] = np.asarray(src[_KLT_HAS_DESC], bool)[st.alive]
    if _KLT_BRIEF in src:  # cfg.klt_corner_describe: so does the BRIEF row
        feats[_KLT_BRIEF] = np.asarray(src[_KLT_BRIEF], np.uint32)[st.alive]
    return feats


def _append_rows(old, extra):
    """``extra`` appended to the rows of ``old`` (numpy or tensor, (N, D) or (1, N, D)), as ``old``'s kind."""
    rows = old[0] if getattr(old, "ndim", 2) == 3 else old
    if hasattr(rows, "detach"):
        import torch

        out = torch.cat([rows, torch.as_tensor(extra, dtype=rows.dtype, device=rows.device)])
    else:
        out = np.concatenate([rows, np.asarray(extra, rows.dtype)])
    return _batched(out, old)


def klt_describe_fallback(st: KltTracker, feats, img, tag):
    """A frame that fell back to detection under ``cfg.klt_corner_describe``: Shi-Tomasi corners of
    its image, at least ``klt_min_distance`` from its detections and from each other, as many as
    ``sift_n_features`` rows leave room for, appended with a zero descriptor, a false flag under
    ``_KLT_HAS_DESC`` and their BRIEF rows under ``_KLT_BRIEF``: what the keyframe's corner rows
    are matched against (:func:`klt_descriptor_rows`)."""
    from .. import brief, corners

    if not isinstance(feats, dict):
        return feats
    kept = np.ascontiguousarray(_keypoints(feats), np.float32).reshape(-1, 2)
    n = len(kept)
    room = max(st.max_rows - n, 0) if st.max_rows > 0 else None
    if room == 0:
        add = np.zeros((0, 2), np.float32)
    else:
        add, _ = corners.good_features(img, room, quality=st.corner_quality, min_distance=st.min_distance,
                                       block_size=st.corner_block, keep=kept, tag=tag)
    rows = brief.describe(img, add, tag=tag)[0] if len(add) else np.zeros((0, brief.WORDS), np.uint32)
    des = feats["descriptors"]
    width = (des[0] if getattr(des, "ndim", 2) == 3 else des).shape[1]
    feats["keypoints"] = _append_rows(feats["keypoints"], add)
    feats["descriptors"] = _append_rows(des, np.zeros((len(add), width), np.float32))
    feats[_KLT_HAS_DESC] = np.concatenate([np.ones(n, bool), np.zeros(len(add), bool)])
    feats[_KLT_BRIEF] = np.concatenate([np.zeros((n, brief.WORDS), np.uint32), rows])
    return feats


def klt_pairs(feats0: dict, feats1: dict):
    """The pairs of a dict tracked from ``feats0`` (``None`` when ``feats1`` is anything else)."""
    if not isinstance(feats1, dict) or feats1.get(_KLT_SRC) is not feats0 or feats0 is None:
        return None
    idx = np.asarray(feats1[_KLT_SRC_IDX], np.int64)
    return np.stack([idx, np.arange(idx.size, dtype=np.int64)], 1)


def far_from(kept: np.ndarray, cand: np.ndarray, dist: float) -> np.ndarray:
    """Which rows of ``cand`` (N, 2) are at least ``dist`` from every row of ``kept`` (M, 2): a grid
    of ``dist``-sized cells over ``kept``, each candidate tested against its 3 x 3 cells."""
    cand = np.asarray(cand, np.float64).reshape(-1, 2)
    kept = np.asarray(kept, np.float64).reshape(-1, 2)
    ok = np.ones(len(cand), bool)
    if not len(kept) or not len(cand) or not dist > 0:
        return ok
    lo = np.floor(min(kept.min(), cand.min()) / dist) - 1
    kc = (np.floor(kept / dist) - lo).astype(np.int64)
    cc = (np.floor(cand / dist) - lo).astype(np.int64)
    W = int(max(kc[:, 0].max(), cc[:, 0].max())) + 2
    kkey = kc[:, 1] * W + kc[:, 0]
    order = np.argsort(kkey, kind="stable")
    kkey, kept = kkey[order], kept[order]
    ckey = cc[:, 1] * W + cc[:, 0]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            a = np.searchsorted(kkey, ckey + dy * W + dx, "left")
            b = np.searchsorted(kkey, ckey + dy * W + dx, "right")
            for j in range(int((b - a).max())):
                i = a + j
                live = i < b
                d = kept[np.minimum(i, len(kept) - 1)] - cand
                ok &= ~(live & ((d * d).sum(1) < dist * dist))
    return ok


def klt_replenish(vo, st: KltTracker, detect) -> int:
    """After a keyframe was made from a tracked frame: detect on its image, keep the detections at
    least ``klt_min_distance`` from every keypoint it has, and append them (evenly thinned to what
    ``sift_n_features`` rows leave room for) with id -1 to ``keyframe["feats"]`` / ``["ids"]``.
    The rows the keyframe had keep their indices.  Returns how many rows were appended."""
    kf = vo.keyframe
    feats = kf.get("feats") if isinstance(kf, dict) else None
    if not isinstance(feats, dict) or feats.get(_KLT_SRC) is None or feats.get(_KLT_IMAGE) is None:
        return 0  # a detected frame is complete already
    if st.corners:
        return klt_replenish_corners(vo, st, feats)
    det = detect(feats[_KLT_IMAGE])
    kept = np.asarray(_keypoints(feats), np.float32).reshape(-1, 2)
    new = np.flatnonzero(far_from(kept, _keypoints(det), st.min_distance))
    room = max(st.max_rows - len(kept), 0) if st.max_rows > 0 else new.size
    if new.size > room:  # evenly over the detector's order, which runs across the image
        new = new[np.linspace(0, new.size - 1, room).round().astype(np.int64)] if room else new[:0]
    kp, des = feats["keypoints"], feats["descriptors"]
    add_kp = _rows(det["keypoints"][0] if getattr(det["keypoints"], "ndim", 2) == 3 else det["keypoints"], new)
    add_des = _rows(_descriptors(det), new)

    def cat(old, add):
        rows = old[0] if getattr(old, "ndim", 2) == 3 else old
        if hasattr(rows, "detach"):
            import torch

            out = torch.cat([rows, torch.as_tensor(add, dtype=rows.dtype, device=rows.device)])
        else:
            out = np.concatenate([rows, np.asarray(_np(add), rows.dtype)])
        return _batched(out, old)

    full = {k: v for k, v in feats.items() if k not in (_KLT_SRC, _KLT_SRC_IDX)}
    full["keypoints"], full["descriptors"] = cat(kp, add_kp), cat(des, add_des)
    ids = np.asarray(kf["ids"])
    kf["feats"] = full
    kf["ids"] = np.concatenate([ids, np.full(new.size, -1, ids.dtype)])
    return int(new.size)


def klt_replenish_corners(vo, st: KltTracker, feats: dict) -> int:
    """:func:`klt_replenish` under ``cfg.klt_corner_replenish``: Shi-Tomasi corners of the keyframe's
    image (its cached pyramid's level 0), at least ``klt_min_distance`` from every keypoint it has
    and from each other, as many as ``sift_n_features`` rows leave room for, strongest first.  Their
    rows get id -1, a zero descriptor and a false flag under ``_KLT_HAS_DESC``.  Under
    ``cfg.klt_corner_describe`` they are also described (:func:`visualodometry_amd.brief.describe`,
    from the keyframe's pyramid tag) and the keyframe keeps (N, 8) uint32 rows under ``_KLT_BRIEF``,
    zeros for the rows that have a descriptor."""
    from .. import corners

    kf = vo.keyframe
    kept = np.ascontiguousarray(_keypoints(feats), np.float32).reshape(-1, 2)
    n_kept = len(kept)
    room = max(st.max_rows - n_kept, 0) if st.max_rows > 0 else None
    if room == 0:
        add = np.zeros((0, 2), np.float32)
    else:
        add, _ = corners.good_features(feats[_KLT_IMAGE], room, quality=st.corner_quality,
                                       min_distance=st.min_distance, block_size=st.corner_block, keep=kept,
                                       tag=feats[_KLT_TAG])
    kp, des = feats["keypoints"], feats["descriptors"]
    des_rows = des[0] if getattr(des, "ndim", 2) == 3 else des

    def cat(old, extra):
        rows = old[0] if getattr(old, "ndim", 2) == 3 else old
        if hasattr(rows, "detach"):
            import torch

            out = torch.cat([rows, torch.as_tensor(extra, dtype=rows.dtype, device=rows.device)])
        else:
            out = np.concatenate([rows, np.asarray(extra, rows.dtype)])
        return _batched(out, old)

    had = np.asarray(feats[_KLT_HAS_DESC], bool) if _KLT_HAS_DESC in feats else np.ones(n_kept, bool)
    full = {k: v for k, v in feats.items() if k not in (_KLT_SRC, _KLT_SRC_IDX)}
    full["keypoints"] = cat(kp, add)
    full["descriptors"] = cat(des, np.zeros((len(add), des_rows.shape[1]), np.float32))
    full[_KLT_HAS_DESC] = np.concatenate([had, np.zeros(len(add), bool)])
    if st.describe:
        from .. import brief

        old = np.asarray(feats[_KLT_BRIEF], np.uint32) if _KLT_BRIEF in feats else \
            np.zeros((n_kept, brief.WORDS), np.uint32)
        new = brief.describe(feats[_KLT_IMAGE], add, tag=feats[_KLT_TAG])[0] if len(add) else old[:0]
        full[_KLT_BRIEF] = np.concatenate([old, new])
    ids = np.asarray(kf["ids"])
    kf["feats"] = full
    kf["ids"] = np.concatenate([ids, np.full(len(add), -1, ids.dtype)])
    return int(len(add))


def klt_descriptor_rows(feats0: dict, feats1: dict, match, brief=None):
    """``match_frames`` between dicts of which one has rows without a descriptor
    (``cfg.klt_corner_replenish``): ``match(sub0, sub1)`` over dicts of the rows that have one, the
    indices mapped back; no pairs from that part when a side has none.  ``None`` when neither dict
    is flagged.

    ``brief`` (``cfg.klt_corner_describe``: the :class:`KltTracker`) adds the pairs of the rows
    without a descriptor when both dicts carry BRIEF rows: ``matcher.match_hamming`` between the two
    sets of corner rows, ratio ``klt_brief_ratio``, ``klt_brief_max_dist`` and the cross check, mapped
    back likewise.  Descriptor rows and corner rows are disjoint on both sides, so the union is as
    one-to-one as its parts; it comes out in ascending keyframe row order."""
    flagged = [isinstance(f, dict) and _KLT_HAS_DESC in f for f in (feats0, feats1)]
    if not any(flagged):
        return None
    rows, subs, empty = [], [], False
    for f, has in zip((feats0, feats1), flagged):
        if not has:
            rows.append(None)
            subs.append(f)
            continue
        idx = np.flatnonzero(np.asarray(f[_KLT_HAS_DESC], bool))
        empty = empty or idx.size == 0
        kp = f["keypoints"]
        sub = {k: v for k, v in f.items() if not k.startswith("_vo_amd_klt")}
        sub["keypoints"] = _batched(_rows(kp[0] if getattr(kp, "ndim", 2) == 3 else kp, idx), kp)
        sub["descriptors"] = _batched(_rows(_descriptors(f), idx), f["descriptors"])
        rows.append(idx)
        subs.append(sub)
    if empty:
        pairs = np.zeros((0, 2), np.int64)
    else:
        pairs = np.asarray(_np(match(subs[0], subs[1])), np.int64).reshape(-1, 2)
        for side in (0, 1):
            if rows[side] is not None:
                pairs[:, side] = rows[side][pairs[:, side]]
    if brief is not None and all(flagged) and _KLT_BRIEF in feats0 and _KLT_BRIEF in feats1:
        from .. import matcher

        crows = [np.flatnonzero(~np.asarray(f[_KLT_HAS_DESC], bool)) for f in (feats0, feats1)]
        if crows[0].size and crows[1].size:
            more = matcher.match_hamming(np.asarray(feats0[_KLT_BRIEF], np.uint32)[crows[0]],
                                         np.asarray(feats1[_KLT_BRIEF], np.uint32)[crows[1]], ratio=brief.brief_ratio,
                                         max_dist=brief.brief_max_dist, cross_check=True)
            more = np.asarray(more, np.int64).reshape(-1, 2)
            both = np.concatenate([pairs, np.stack([crows[0][more[:, 0]], crows[1][more[:, 1]]], 1)])
            pairs = both[np.argsort(both[:, 0], kind="stable")]
    return pairs


def _detect_as_today(frontend, image):
    """``process_image`` of ``frontend`` without the route: the wrapped method's detection path when
    the hooks are installed, else the class's own method."""
    pi = type(frontend).process_image
    return getattr(pi, "_vo_amd_detect", pi)(frontend, image)


def run_window_ba(vo, win: KeyframeWindow):
    """Adjust the window and write poses/points back into the VO state; never raises on bad windows."""
    window, lm_ids = win.build(vo.map_points)
    if window is None:
        return None
    cfg = vo.cfg
    ba = getattr(vo, "_vo_amd_ba", None)
    if ba is None:
        ba = SlidingWindowBA(vo.K, cfg)
        vo._vo_amd_ba = ba
    # cfg.ba_covariance: the result (kept on vo._vo_amd_last_ba) also carries the pose and landmark
    # covariance of the adjusted window; no policy here reads it
    # cfg.ba_marginalize: a full window also computes the prior its oldest keyframe leaves behind
    kw = {}
    if getattr(cfg, "ba_covariance", False):
        kw["return_covariance"] = True
    marg = bool(getattr(cfg, "ba_marginalize", False))  # (off: nothing of the window but build / write_back is used)
    slide = marg and win.full()
    if slide:
        kw["marginalize"] = 1
    res = ba.optimize(window, **kw)
    if res.status != "ok" or not np.all(np.isfinite(res.cost_per_iter)) or \
            res.cost_per_iter[-1] > res.cost_per_iter[0]:
        print(f"BA: window rejected ({res.status} {res.message})")
        if marg:  # what the prior was linearised around is no longer trusted
            win.clear_prior()
            win.marginalised.clear()
        return res
    win.write_back(res, lm_ids, vo.map_points, window.obs_pt)
    if slide:
        if res.prior is not None and res.point_marginalised is not None:
            win.slide(res.prior, np.asarray(lm_ids)[res.point_marginalised])
        else:  # the elimination failed: the next window starts without a prior
            win.clear_prior()
    T_wc = win.frames[-1].T_wc.copy()
    vo.T_wc = T_wc
    vo.keyframe["T_wc"] = T_wc.copy()
    vo.last_pos = T_wc[:3, 3].copy()
    return res


def _use_map_store(vo) -> None:
    if getattr(vo.cfg, "map_store_arrays", True) and not isinstance(vo.map_points, MapStore):
        store = MapStore()
        for pid, X in vo.map_points.items():
            store[pid] = X
        vo.map_points = store


def _wrap_init(orig):
    def __init__(self, *args, **kw):  # VisualOdometry(K, config), vo.py:9
        orig(self, *args, **kw)
        _PNP_ON_GPU[0] = bool(getattr(self.cfg, "pnp_on_gpu", True))
        _INIT_ON_GPU[0] = bool(getattr(self.cfg, "init_on_gpu", False))
        _use_map_store(self)
        st = getattr(getattr(self, "frontend", None), "_vo_amd_klt", None)
        if st is not None:  # cfg.klt_tracking: the frontend tracks from its owner's keyframe
            st.owner = weakref.ref(self)
        if getattr(self.cfg, "ba_enabled", False):
            # the BA context pre-sized for a full window (ba_window keyframes, the map's
            # MAX_POINTS cap, vo.py:38) now, so no keyframe call of the drive pays for it
            self._vo_amd_ba = SlidingWindowBA(self.K, self.cfg)
            self._vo_amd_ba.reserve(getattr(self.cfg, "ba_window", 50), MAX_POINTS,
                                    n_fixed=getattr(self.cfg, "ba_fixed", 2))

    __init__._vo_amd_wrapped = orig
    return __init__


def _wrap_prune(orig):
    def _prune_map(self):
        if isinstance(self.map_points, MapStore):
            self.map_points.prune_below(self.next_pt_id - MAX_POINTS)  # vo.py:38-47
        else:
            orig(self)
        store = getattr(self, "_vo_amd_lm_desc", None)
        if store is not None:  # cfg.map_reobserve: the descriptors leave with their landmarks
            store.prune_below(self.next_pt_id - MAX_POINTS)

    _prune_map._vo_amd_wrapped = orig
    return _prune_map


def _wrap_reset(orig):
    def _reset_system(self):
        orig(self)
        _use_map_store(self)
        win = getattr(self, "_vo_amd_window", None)
        if win is not None:
            win.reset()
        store = getattr(self, "_vo_amd_lm_desc", None)
        if store is not None:
            store.clear()
        st = getattr(getattr(self, "frontend", None), "_vo_amd_klt", None)
        if st is not None:
            st.reset()

    _reset_system._vo_amd_wrapped = orig
    return _reset_system


_PNP_ON_GPU = [True]  # set from the VO config at construction (cfg.pnp_on_gpu)
_INIT_ON_GPU = [False]  # likewise cfg.init_on_gpu (findEssentialMat + recoverPose, vo.py:87-101)


def _wrap_frontend_init(orig):
    from .. import sift

    def __init__(self, config, *args, **kw):  # FeatureFrontend(config), frontend.py:10
        orig(self, config, *args, **kw)
        if getattr(config, "extractor_type", None) == "sift" and getattr(config, "sift_on_gpu", True):
            self.extractor = sift.SIFT_create(nfeatures=config.sift_n_features,
                                              contrastThreshold=config.sift_contrast_threshold,
                                              edgeThreshold=config.sift_edge_threshold, sigma=config.sift_sigma)
        # the KLT tracking front end (SIFT extractor only): its settings are read here, once, so the
        # frame path of a frontend without the route reads no klt_* setting at all
        if getattr(config, "extractor_type", None) == "sift" and getattr(config, "klt_tracking", False):
            self._vo_amd_klt = KltTracker(config)

    __init__._vo_amd_wrapped = orig
    return __init__


def _wrap_process_image(orig):
    from .. import sift

    def process_image(self, img):  # FeatureFrontend.process_image, frontend.py:36-75
        st = self.__dict__.get("_vo_amd_klt")  # cfg.klt_tracking (off: not set, nothing below runs)
        if st is not None:
            return klt_process_image(st, img, lambda: detect(self, img))
        return detect(self, img)

    def detect(self, img):  # the frame path without the route
        ext = getattr(self, "extractor", None)
        dev = getattr(self, "device", None)
        if isinstance(ext, sift.SIFT) and getattr(dev, "type", None) == "cuda" and np.ndim(img) == 2:
            # the SIFT branch (:51-75) keeps k.pt and the descriptors and moves both to the GPU:
            # the kernels write them into torch's memory there, no keypoint objects on the host
            import torch

            r = sift.detect_and_compute_torch(img, ext.nfeatures, ext.contrast, ext.edge, ext.sigma, ext.n_layers,
                                              device=dev, ctx=ext._ctx or None)
            if r is not None:
                pts, des = r
                return {
                    "keypoints": pts.unsqueeze(0),  # (1, N, 2)
                    "descriptors": des.unsqueeze(0),  # (1, N, 128)
                    "image_size": torch.tensor([(img.shape[1], img.shape[0])]).to(dev),
                }
        return orig(self, img)

    process_image._vo_amd_wrapped = orig
    process_image._vo_amd_detect = detect
    return process_image


def _wrap_match_frames(orig):
    from .. import matcher

    def match_frames(self, feats0, feats1):
        if self.__dict__.get("_vo_amd_klt") is not None:  # cfg.klt_tracking: a tracked frame brings its pairs
            pairs = klt_pairs(feats0, feats1)
            if pairs is not None:
                return pairs
            st = self.__dict__["_vo_amd_klt"]
            pairs = klt_descriptor_rows(feats0, feats1, lambda a, b: plain(self, a, b),  # cfg.klt_corner_replenish
                                        st if st.describe else None)  # cfg.klt_corner_describe
            if pairs is not None:
                return pairs
        return plain(self, feats0, feats1)

    def plain(self, feats0, feats1):  # the matching without the route
        if getattr(self.conf, "extractor_type", None) == "sift" and getattr(self.conf, "match_on_gpu", True):
            # SIFT integers: the int8 path only, hinted for this call (the context's own hint,
            # which other users of the context may rely on, is restored afterwards)
            # feats0 is the keyframe's (vo.py:64-65): its packed rows stay cached across frames
            return matcher.match_knn2_ratio(feats0["descriptors"], feats1["descriptors"],
                                            kind=matcher.DESC_SIFT, cache_query=True,
                                            cross_check=bool(getattr(self.conf, "match_cross_check", False)))
        if getattr(self.conf, "extractor_type", None) == "superpoint" and \
                getattr(self.conf, "superpoint_bf_match", False):
            # BASELINE config 5: brute force in place of LightGlue (frontend.py:77-84).  The VO loop
            # indexes keyframe["ids"][ref_indices] (vo.py:66,121), so the pairs must be one-to-one
            # as LightGlue's are: ratio test + cross check.  The dicts' (1, N, 256) CUDA tensors
            # are read in place; the result is the (M, 2) int64 array that branch returns
            return matcher.match_knn2_ratio(feats0["descriptors"], feats1["descriptors"],
                                            ratio=float(getattr(self.conf, "superpoint_bf_ratio", 0.75)),
                                            kind=matcher.DESC_FLOAT, cache_query=True, cross_check=True)
        return orig(self, feats0, feats1)

    match_frames._vo_amd_wrapped = orig
    return match_frames


def _wrap_triangulate(orig):
    from .. import triangulate

    def triangulate_points(T_cw1, T_cw2, pts1, pts2, K, config):
        if getattr(config, "triangulate_on_gpu", True):
            return triangulate.triangulate_points(T_cw1, T_cw2, pts1, pts2, K, config)
        return orig(T_cw1, T_cw2, pts1, pts2, K, config)

    triangulate_points._vo_amd_wrapped = orig
    return triangulate_points


class Cv2Proxy:
    """Stands in for the ``cv2`` module inside ``modules.vo``: ``solvePnPRansac`` runs on
    the MI355X, and so do ``findEssentialMat`` and ``recoverPose`` of the initialisation
    (``vo.py:87-101``) when ``init_enabled()``; every other attribute is the real cv2's."""

    def __init__(self, real, enabled=lambda: True, init_enabled=lambda: False):
        self._vo_amd_real = real
        self._enabled = enabled
        self._init_enabled = init_enabled

    def __getattr__(self, name):
        return getattr(self._vo_amd_real, name)

    def solvePnPRansac(self, objectPoints, imagePoints, cameraMatrix, distCoeffs=None, *args, **kw):
        if self._enabled():
            from .. import pnp

            return pnp.solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, *args, **kw)
        return self._vo_amd_real.solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, *args, **kw)

    def findEssentialMat(self, points1, points2, *args, **kw):
        if self._init_enabled():
            from .. import essential

            if kw.get("method") == getattr(self._vo_amd_real, "RANSAC", essential.RANSAC):
                kw["method"] = essential.RANSAC
            return essential.findEssentialMat(points1, points2, *args, **kw)
        return self._vo_amd_real.findEssentialMat(points1, points2, *args, **kw)

    def recoverPose(self, E, points1, points2, *args, **kw):
        if self._init_enabled():
            from .. import essential

            return essential.recoverPose(E, points1, points2, *args, **kw)
        return self._vo_amd_real.recoverPose(E, points1, points2, *args, **kw)


def install(frontend_cls=None, vo_cls=None) -> None:
    """Patch the reference classes (imported from ``modules.*`` when not given). Idempotent.

    ``triangulate_points`` (``frontend.py:115``) is a module function that ``vo.py``
    imports by name (``vo.py:6``), so it is replaced in both modules.
    """
    import sys

    if frontend_cls is None:
        from modules.frontend import FeatureFrontend as frontend_cls  # the reference's module
    if vo_cls is None:
        from modules.vo import VisualOdometry as vo_cls
    for name in dict.fromkeys((frontend_cls.__module__, vo_cls.__module__)):
        mod = sys.modules.get(name)
        f = getattr(mod, "triangulate_points", None) if mod is not None else None
        if f is not None and not hasattr(f, "_vo_amd_wrapped"):
            mod.triangulate_points = _wrap_triangulate(f)
    if not hasattr(frontend_cls.__init__, "_vo_amd_wrapped"):
        frontend_cls.__init__ = _wrap_frontend_init(frontend_cls.__init__)
    if not hasattr(frontend_cls.match_frames, "_vo_amd_wrapped"):
        frontend_cls.match_frames = _wrap_match_frames(frontend_cls.match_frames)
    pi = getattr(frontend_cls, "process_image", None)
    if pi is not None and not hasattr(pi, "_vo_amd_wrapped"):
        frontend_cls.process_image = _wrap_process_image(pi)
    if not hasattr(vo_cls._create_keyframe, "_vo_amd_wrapped"):
        vo_cls._create_keyframe = _wrap_create_keyframe(vo_cls._create_keyframe)
    if not hasattr(vo_cls._reset_system, "_vo_amd_wrapped"):
        vo_cls._reset_system = _wrap_reset(vo_cls._reset_system)
    if not hasattr(vo_cls.__init__, "_vo_amd_wrapped"):
        vo_cls.__init__ = _wrap_init(vo_cls.__init__)
    if hasattr(vo_cls, "_prune_map") and not hasattr(vo_cls._prune_map, "_vo_amd_wrapped"):
        vo_cls._prune_map = _wrap_prune(vo_cls._prune_map)
    vo_mod = sys.modules.get(vo_cls.__module__)
    real_cv2 = getattr(vo_mod, "cv2", None) if vo_mod is not None else None
    if real_cv2 is not None and not isinstance(real_cv2, Cv2Proxy):
        vo_mod.cv2 = Cv2Proxy(real_cv2, lambda: _PNP_ON_GPU[0], lambda: _INIT_ON_GPU[0])
