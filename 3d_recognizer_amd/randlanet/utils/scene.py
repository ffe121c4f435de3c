"""Voted-crop inference over a whole scene (Model.predict_scene): RandLA-Net's test protocol (Hu et al., CVPR 2020; the
authors' S3DIS / Semantic3D testers) - a "possibility" per point, crops of the n nearest neighbours of the least covered
point, the softmax of every crop blended into a per-point probability - for clouds much larger than settings.n_points.

This module is the numpy host twin of csrc/scene.hip (include/rl_randlanet.h, rl_scene_*): a model placed on the CPU runs
predict_scene through it, and the GPU tests compare the kernels against it.  The crop sequence only depends on integer
work and on fixed float32 expressions, so the twin and the kernels pick the same crops bit for bit.
"""
from typing import Optional, Tuple

import numpy as np

_F32 = np.float32


def initial_possibility(M: int, seed: int) -> np.ndarray:
    """Possibilities of a fresh scene: small random values from a private generator (the global numpy stream is not used)."""
    return np.random.default_rng(seed).random(M, dtype=np.float32) * _F32(1e-3)


def pick(possibility: np.ndarray) -> int:
    """The next crop centre: the least covered point, ties to the lowest index."""
    return int(np.argmin(possibility))


def squared_distances(xyz: np.ndarray, c: int) -> np.ndarray:
    """d2_i = ((dx*dx)+(dy*dy))+(dz*dz) in float32, each operation rounded (the KNN's expression)."""
    d = xyz[c].astype(_F32) - xyz.astype(_F32, copy=False)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def select(d2: np.ndarray, n: int) -> Tuple[np.ndarray, np.float32]:
    """Indices of the n smallest keys (d2_i, i) in ascending index order, and the largest d2 among them."""
    M = d2.shape[0]
    assert 0 < n <= M, f"crop of {n} points out of {M}"
    T = np.partition(d2, n - 1)[n - 1]
    lt = d2 < T
    take_eq = n - int(np.count_nonzero(lt))
    sel = lt
    eq = np.flatnonzero(d2 == T)[:take_eq]
    sel[eq] = True
    return np.flatnonzero(sel), _F32(T)


def update(possibility: np.ndarray, idx: np.ndarray, d2: np.ndarray, dmax: np.float32) -> None:
    """possibility[idx] += (1 - d2/dmax)^2 in float32 (dmax == 0: every crop point is at the centre, delta 1)."""
    r = d2 / dmax if dmax != 0 else np.zeros_like(d2)
    t = _F32(1) - r
    possibility[idx] = possibility[idx] + t * t


def padded_select(d2: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray, np.float32]:
    """The padded crop's selection out of M = len(d2) keys: (the points whose possibility rises, the n slots, d2max).
    M >= n: select(d2, n), slots and points the same.  M < n: every point (d2max the largest d2 of the scene), and slot j
    holds point j mod M - the points ascending, then repeated cyclically.  (The authors fill a small cloud up with
    np.random.choice; cyclic repeats are a deliberate deviation: every point weighs the same within one repeat, and no
    random stream enters the crop sequence.)"""
    idx, dmax = select(d2, min(n, d2.shape[0]))
    return idx, np.resize(idx, n), dmax


def crop(cloud: np.ndarray, possibility: np.ndarray, n: int, pad: bool = False) -> np.ndarray:
    """One crop of rl_scene_crop: pick, select, update (in place).  Returns the crop's point indices, ascending.
    pad: one crop of rl_scene_crop_padded - n may exceed the M points of the cloud; then every possibility rises once and
    the n slots are np.resize(arange(M), n) (padded_select)."""
    c = pick(possibility)
    d2 = squared_distances(cloud[:, :3], c)
    if pad:
        idx, slots, dmax = padded_select(d2, n)
    else:
        idx, dmax = select(d2, n)
        slots = idx
    update(possibility, idx, d2[idx], dmax)
    return slots


def softmax_cf(logits: np.ndarray) -> np.ndarray:
    """Softmax over axis 0 of (C, n) float32 logits (rl_softmax_cf's expression)."""
    z = logits.astype(_F32, copy=False)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def exp_fixed(x: np.ndarray) -> np.ndarray:
    """e^x of float32 x <= 0 as the fixed sequence of float32 operations of scene.hip's exp_fixed, bit for bit:
    k = rint(x*log2(e)), r = x - k*ln2 in two steps, the degree-5 polynomial of Cephes' expf (1.7e-7 relative) by Horner in
    separate multiplies and adds, times 2^k.  Below -87, and for NaN, it is 0."""
    x = np.asarray(x, _F32)
    with np.errstate(invalid="ignore"):
        live = x >= _F32(-87)
    x = np.where(live, x, _F32(0))
    k = np.rint(x * _F32(1.44269504088896341))
    r = x - k * _F32(0.693359375)
    r = r - k * _F32(-2.12194440e-4)
    p = np.full_like(r, _F32(1.9875691500e-4))
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * r + _F32(c)
    p = (p * (r * r) + r) + _F32(1)
    two_k = ((k.astype(np.int32) + 127) << 23).view(_F32)
    return np.where(live, p * two_k, _F32(0))


def softmax_fixed(logits: np.ndarray) -> np.ndarray:
    """Softmax over axis 0 of (C, n) float32 logits by exp_fixed, the classes summed in order: the bits of
    rl_scene_accumulate_first."""
    z = logits.astype(_F32, copy=False)
    e = exp_fixed(z - z.max(axis=0, keepdims=True))
    den = np.zeros(z.shape[1], _F32)
    for c in range(z.shape[0]):
        den = den + e[c]
    return e / den


def accumulate(prob: np.ndarray, count: np.ndarray, logits: np.ndarray, idx: np.ndarray, one_minus_s: np.float32,
               s: np.float32, first: int = None) -> None:
    """rl_scene_accumulate: prob (M, C) of the crop's points <- s*prob + (1-s)*softmax, count += 1 (idx duplicate-free).
    first: rl_scene_accumulate_first - only the first `first` slots of the crop are blended and counted (those of a padded
    crop that are duplicate-free: a point is voted once per crop), and the softmax is softmax_fixed, whose bits the kernel
    reproduces (softmax_cf's np.exp and the device's expf agree to a few 1e-7 only)."""
    if first is not None:
        logits, idx = logits[:, :first], idx[:first]
    sm = (softmax_cf(logits) if first is None else softmax_fixed(logits)).T
    prob[idx] = s * prob[idx] + one_minus_s * sm
    count[idx] += 1


def blend_factors(smooth: float) -> Tuple[np.float32, np.float32]:
    """(s, 1 - s) as float32; 1 - s is computed once, then rounded."""
    return _F32(smooth), _F32(1.0 - smooth)


def normalise(prob: np.ndarray) -> np.ndarray:
    """(M, C) blended probabilities -> (C, M) confidences whose columns sum to 1."""
    return np.ascontiguousarray((prob / prob.sum(axis=1, keepdims=True)).T)


# --------------------------------------------------------------------------------------- training crops over many scenes
# The twin of rl_scenes_crop (Model.train_scenes): RandLA-Net's training sampler (the authors' spatially_regular_gen) over
# S scenes concatenated into one array, scene s owning rows [off[s], off[s+1]).


def scene_offsets(sizes) -> np.ndarray:
    """off (S+1) int64 of scenes with `sizes` points, off[0] = 0."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def scenes_pick(possibility: np.ndarray, off: np.ndarray) -> Tuple[int, int]:
    """(g, s): the least (possibility, row) over all scenes and the scene that holds it."""
    g = int(np.argmin(possibility))
    return g, int(np.searchsorted(off, g, side="right") - 1)


def centre_noise(center_noise: float) -> np.ndarray:
    """The centre offset of one crop as float32: three np.random.normal draws when center_noise > 0, none otherwise."""
    if center_noise > 0:
        return np.random.normal(0, center_noise, 3).astype(_F32)
    return np.zeros(3, _F32)


def scenes_crop(xyz: np.ndarray, off: np.ndarray, possibility: np.ndarray, n: int,
                noise: np.ndarray = None, pad: bool = False) -> Tuple[int, np.ndarray]:
    """One crop of rl_scenes_crop over float32 xyz (T, 3): pick, select inside the picked scene, update (in place).
    Returns (scene, the crop's GLOBAL rows ascending).  pad: one crop of rl_scenes_crop_padded - a picked scene of fewer
    than n points is taken whole, raised once, and repeated cyclically over the n slots (padded_select)."""
    g, s = scenes_pick(possibility, off)
    b, e = int(off[s]), int(off[s + 1])
    p = xyz[g].astype(_F32)
    if noise is not None:
        p = p + noise.astype(_F32)
    d = p - xyz[b:e].astype(_F32, copy=False)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    if pad:
        idx, slots, dmax = padded_select(d2, n)
    else:
        idx, dmax = select(d2, n)
        slots = idx
    update(possibility[b:e], idx, d2[idx], dmax)
    return s, slots + b


# ------------------------------------------------------------------------------------------ voted crops over many scenes
# The twin of rl_scenes_vote_crop / rl_scenes_vote_accumulate (Model.predict_scenes): the sampler above competing for
# coverage.  count (T) int32 holds the crops every point was in; scene s is open while its least count is below `votes`.


def scenes_low(off: np.ndarray, count: np.ndarray) -> np.ndarray:
    """low (S) int32 of rl_scenes_vote_crop: the least count of every scene."""
    return np.array([count[off[s]:off[s + 1]].min() for s in range(len(off) - 1)], np.int32)


def scenes_vote_crop(xyz: np.ndarray, off: np.ndarray, possibility: np.ndarray, count: np.ndarray, votes: int, n: int,
                     pad: bool = False) -> Optional[Tuple[int, np.ndarray, int]]:
    """One crop of rl_scenes_vote_crop: g = the least (possibility, row) over the OPEN scenes only, then scenes_crop's
    select and update inside its scene (no centre noise), and count += 1 for every selected point - once per point, the
    cyclic repeats of a padded crop do not count.  The count rises here, at crop time, so the next crop of the same pass
    already sees a covered scene closed.  Returns (scene, the n slots' GLOBAL rows, first) with first = min(n, M_s) the
    leading duplicate-free slots, or None when no scene is open: the slot is idle and nothing changes."""
    low = scenes_low(off, count)
    best = None
    for s in np.flatnonzero(low < votes):
        b, e = int(off[s]), int(off[s + 1])
        g = b + int(np.argmin(possibility[b:e]))
        if best is None or (possibility[g], g) < best[0]:
            best = ((possibility[g], g), int(s))
    if best is None:
        return None
    (_, g), s = best
    b, e = int(off[s]), int(off[s + 1])
    d = xyz[g, :3].astype(_F32) - xyz[b:e, :3].astype(_F32, copy=False)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    if pad:
        idx, slots, dmax = padded_select(d2, n)
    else:
        idx, dmax = select(d2, n)
        slots = idx
    update(possibility[b:e], idx, d2[idx], dmax)
    count[b + idx] += 1
    return s, slots + b, len(idx)


def scenes_vote_accumulate(prob: np.ndarray, logits: np.ndarray, idx: np.ndarray, one_minus_s: np.float32, s: np.float32,
                           first: int) -> None:
    """One slot of rl_scenes_vote_accumulate: accumulate(..., first=first) on global rows without its count update (the
    count rose at crop time); always softmax_fixed.  first == 0 (an idle slot) changes nothing."""
    if first <= 0:
        return
    idx = idx[:first]
    prob[idx] = s * prob[idx] + one_minus_s * softmax_fixed(logits[:, :first]).T
