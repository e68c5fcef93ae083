"""Frames of the ORB selection tests (test_orb_select_cases.py, test_gpu_orb_select.py): inputs that
put select_kernel (mageslam_amd/csrc/orb.hip) on the branches the synthetic sequence never reaches,
and a NumPy restatement of the counts that decide those branches.  Not a test module (nothing is
collected); nothing here touches the GPU.

    n0   candidates of a level: strict 3x3 maxima of the FAST score map inside the border
    cut  RetainBestFeatures (OpenCVModified.cpp:571-617): with more than N candidates, a suffix
         histogram of the responses gives minNumThreshold (the largest response with at least N
         candidates at or above it, at least t), lower = max((int)(f32(minNumThreshold) *
         f32(strength)), t) and cut = max(hiM, lower), hiM the largest response with at least
         (int)(f32(N) * f32(factor)) candidates at or above it
    K    candidates with response >= cut: what ANMS ranks (all of them when n0 <= N)

select_kernel holds K <= KMAX items in LDS, sorts (minR2, response, ~raster) keys, takes the ANMS
path when n0 > N and K >= N, and reads one candidate slot per FAST tile (TILE_W x TILE_H pixels).
"""
from __future__ import annotations

import functools

import numpy as np

from mageslam_amd import synth

KMAX = 8192
TILE_W, TILE_H = 120, 30
SEL_THREADS = 1024
REDO_WORKGROUPS = 8


def dots(w, h, px, py, val=200, bg=100, limit=None, x0=10, y0=10):
    """Single bright pixels on the lattice (x0 + i px, y0 + j py) over a flat background, kept
    x0 / y0 away from the right / bottom side.  `val` is a level or a function of the lattice
    coordinates (X, Y); `limit` keeps the first dots in raster order."""
    img = np.full((h, w), bg, np.uint8)
    Y, X = np.meshgrid(np.arange(y0, h - y0, py), np.arange(x0, w - x0, px), indexing="ij")
    v = val(X, Y) if callable(val) else np.full(X.shape, val)
    X, Y, v = X.ravel()[:limit], Y.ravel()[:limit], np.asarray(v).ravel()[:limit]
    img[Y, X] = v
    return img


def mixed_val(X, Y):
    """One dot in six at 220, the rest at 170."""
    return np.where(((Y - 10) // 10 + 3 * ((X - 10) // 11)) % 6 == 0, 220, 170)


def tiles(w, h):
    return ((w + TILE_W - 1) // TILE_W) * ((h + TILE_H - 1) // TILE_H)


def _oracle():
    from oracle import oracle as O  # the CPU oracle (tests only); built by the `oracle` fixture

    return O


def candidates(img, t=4, border=7):
    """(x, y, response) of the strict 3x3 maxima of the oracle's FAST score map with
    border <= x < w - border and border <= y < h - border, in raster order."""
    s = _oracle().fast_score_map(img, t).astype(np.int32)
    h, w = s.shape
    b = max(border, 3)
    if h <= 2 * b or w <= 2 * b:
        z = np.zeros(0, np.int32)
        return z, z, z
    c = s[b:h - b, b:w - b]
    m = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                m &= c > s[b + dy:h - b + dy, b + dx:w - b + dx]
    y, x = np.nonzero(m)
    return (x + b).astype(np.int32), (y + b).astype(np.int32), c[y, x]


def retain(scores, N, t=4, feature_factor=1.5, feature_strength=0.9):
    """(n0, cut, K) of one level by the RetainBestFeatures rule (cut 0 when nothing is cut)."""
    scores = np.asarray(scores, np.int64)
    n0 = len(scores)
    if n0 <= N:
        return n0, 0, n0
    sfx = np.cumsum(np.bincount(np.clip(scores, 0, 255), minlength=256)[::-1])[::-1]  # sfx[i]: responses >= i
    max_num = int(np.float32(N) * np.float32(feature_factor))
    reach = np.nonzero(sfx[t:] >= N)[0]
    min_num_threshold = t + int(reach[-1]) if len(reach) else t
    lower = max(int(np.float32(min_num_threshold) * np.float32(feature_strength)), t)
    reach = np.nonzero(sfx[lower:] >= max_num)[0]
    cut = lower + int(reach[-1]) if len(reach) else lower
    return n0, cut, int(sfx[cut])


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


PYRAMID = dict(nlevels=4, patch_size=31, use_orientation=True)  # oracle.default_settings keywords
PYRAMID3 = dict(nlevels=3, patch_size=31, use_orientation=True)

# name -> (frame builder, NumFeatures)
_CASES = {
    "ties": (lambda: dots(1280, 720, 11, 10, val=200), 2000),
    "kmax": (lambda: dots(1280, 720, 10, 10, val=200, limit=KMAX), 2000),
    "kmax+1": (lambda: dots(1280, 720, 10, 10, val=200, limit=KMAX + 1), 2000),
    "mixed": (lambda: dots(1280, 720, 11, 10, val=mixed_val), 2000),
    "row": (lambda: dots(1280, 64, 4, 1000, y0=30), 100),
    "col": (lambda: dots(64, 1280, 1000, 4, x0=30), 100),
    "thin_w": (lambda: noise(4095, 40, 1), 500),
    "thin_h": (lambda: noise(40, 4095, 2), 500),
    "hd": (lambda: synth.frame(0, 1920, 1080), 2000),
    "cap_in_level": (lambda: synth.frame(0, 640, 480), 2000),
    "cells": (lambda: synth.frame(2, 640, 480), 1000),
}
PARITY = ("ties", "kmax", "mixed", "row", "col", "thin_w", "thin_h", "hd")
BATCH_PARITY = ("ties", "mixed", "hd")
CAP_IN_LEVEL = (900, 1200)
REDO_W, REDO_H, REDO_N, REDO_FRAMES = 320, 180, 300, 20
REDO_GATE, BLANK_GATE = 250, 60
REDO_BLANK = (1, 2, 4, 5, 7, 8, 10, 11, 13, 15, 17, 19)  # the 12 frames of the mixed list replaced by a flat one


@functools.lru_cache(maxsize=None)
def frame(name):
    img = np.ascontiguousarray(_CASES[name][0]())
    img.setflags(write=False)
    return img


def nfeatures(name):
    return _CASES[name][1]


@functools.lru_cache(maxsize=None)
def plain(w, h, t=1):
    """An ordinary frame a tie-heavy one shares a batch with."""
    img = synth.frame(t, w, h)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def redo_frames(blank=False):
    f = np.stack([synth.frame(t, REDO_W, REDO_H) for t in range(REDO_FRAMES)])
    if blank:
        f[list(REDO_BLANK)] = 128
    f.setflags(write=False)
    return f


_oracle_out = {}


def expected(img_key, img, settings_kw, nfeat, cap=None):
    """The oracle's (keypoints, descriptors) for a frame, computed once per (frame, settings)."""
    key = (img_key, nfeat, cap, tuple(sorted(settings_kw.items())))
    if key not in _oracle_out:
        O = _oracle()
        st, kp, d = O.orb_detect(img, O.default_settings(nfeat, **settings_kw), cap=cap)
        assert st == 0, key
        kp.setflags(write=False)
        d.setflags(write=False)
        _oracle_out[key] = (kp, d)
    return _oracle_out[key]


def expected_case(name, cap=None, **settings_kw):
    return expected(name, frame(name), settings_kw, nfeatures(name), cap)
