"""Windows, maps and references shared by the window palette tests (CPU and GPU):
the expected dominant slot in plain numpy (the counts are
tests/box_palette_cases.expected_counts), the host twin's call, the window lists,
the slot-count edges and the special windows.  Every comparison is integer for
integer and leaves no window out."""
import ctypes

import numpy as np

from tests import box_palette_cases as bpc
from tests.window_sharp_cases import ODD_H, ODD_W, SIZES, boundaries, odd_windows   # noqa: F401

NONE = bpc.NONE
MAX_SLOTS = 4096
# pal_window.h's copies rule: 16 (4 at 16 and 32 px) copies halved until copies *
# (n_slots + 1) <= 2048 -- it changes where n_slots + 1 passes 128, 256, 512, 1024
COPY_THRESHOLDS = (128, 256, 512, 1024)
SLOT_EDGES = (0, 1, 17, 4096, 127) + tuple(c + d for c in COPY_THRESHOLDS for d in (-1, 0))


def expected_dominant(counts, n_slots):
    """uint16 [n]: the first column of the largest count, column n_slots as NONE."""
    counts = np.asarray(counts)
    assert counts.shape[-1] == n_slots + 1
    col = np.argmax(counts, axis=-1)
    return np.where(col == n_slots, NONE, col).astype(np.uint16)


def edge_windows(T, h, w):
    """Windows of an h x w map with left = 0, 1, 2, 3 (mod 4) where they fit, flush
    to all four edges and in the bottom-right corner, two overlapping, the second
    twice more at the end."""
    wins = [(0, T, l, l + T) for l in (0, 1, 2, 3) if l + T <= w]
    wins += [(h - T, h, 0, T), (0, T, w - T, w), (h - T, h, w - T, w), ((h - T) // 2, (h - T) // 2 + T, w - T, w),
             (h - T, h, (w - T) // 2, (w - T) // 2 + T)]
    if h - T >= 2 and w - T >= 6:
        wins += [(1, 1 + T, 5, 5 + T), (2, 2 + T, 6, 6 + T)]          # overlapping
    wins += [wins[1 % len(wins)]] * 2
    return wins


def all_windows(T, h, w):
    """Every T x T window of an h x w map, row-major: the grid at stride 1."""
    return [(y, y + T, x, x + T) for y in range(h - T + 1) for x in range(w - T + 1)]


def host_twin(lab, boxes, n_slots, T, counts=True, dominant=True, fill=None):
    """phd_debug_window_palette_host over a uint16 map (any 2-byte aligned base):
    (counts [n, n_slots + 1] uint32, dominant [n] uint16) -- an output not asked
    for comes back as it went in (`fill`) -- or the error text."""
    from photohive_dsp_amd import lib as L
    assert lab.dtype == np.uint16 and lab.flags.c_contiguous
    cb = boundaries(boxes)
    n = len(boxes)
    c = np.full((n, max(n_slots, 0) + 1), 0xDEADBEEF if fill is None else fill, np.uint32)
    d = np.full(n, 0xBEEF if fill is None else fill & 0xFFFF, np.uint16)
    rc = L.lib.phd_debug_window_palette_host(lab.ctypes.data, lab.shape[0], lab.shape[1], n_slots, ctypes.byref(cb), T,
                                             c.ctypes.data if counts else None, d.ctypes.data if dominant else None)
    if rc != 0:
        assert rc == -1
        return L.last_error()
    return c, d


def expected(lab, boxes, n_slots):
    c = bpc.expected_counts(lab, boxes, n_slots)
    return c, expected_dominant(c, n_slots)


def odd_map(n_slots=17, seed=5):
    """The 131 x 197 map: the odd width puts every row at another phase."""
    return bpc.random_map(ODD_H, ODD_W, n_slots, seed)


# ---- special windows: (name, n_slots, T x T labels, expected dominant) -----------------------------
SPECIALS = ("single", "alternating", "all_none", "over", "half_2_5", "half_none_3", "none_majority")


def special_window(name, T):
    """(n_slots, the window's T x T uint16 labels, its dominant label)."""
    n = T * T
    flat = np.zeros(n, np.uint16)
    if name == "single":                             # one counter is T^2
        flat[:] = 9
        return 17, flat.reshape(T, T), 9
    if name == "alternating":                        # no runs to merge; a tie of 4 and 11: the lower
        flat[:] = np.where(np.arange(n) % 2 == 0, 11, 4)
        return 17, flat.reshape(T, T), 4
    if name == "all_none":
        flat[:] = NONE
        return 17, flat.reshape(T, T), NONE
    if name == "over":                               # labels >= n_slots that are not NONE: the last column
        flat[:] = np.where(np.arange(n) % 3 == 0, 17, 40000)
        return 17, flat.reshape(T, T), NONE
    if name == "half_2_5":                           # a tie: the lower slot
        flat[:n // 2], flat[n // 2:] = 5, 2
        return 17, flat.reshape(T, T), 2
    if name == "half_none_3":                        # none wins only when strictly larger
        flat[:n // 2], flat[n // 2:] = NONE, 3
        return 17, flat.reshape(T, T), 3
    if name == "none_majority":
        flat[:n // 2 + 1], flat[n // 2 + 1:] = NONE, 3
        return 17, flat.reshape(T, T), NONE
    raise KeyError(name)


def special_map(T):
    """The special windows side by side, one label column apart (so their lefts
    take every phase), in a map of NONE + 1 ... : (map, boxes, n_slots, dominants)."""
    k = len(SPECIALS)
    lab = np.full((T + 2, k * (T + 1) + 3), 16, np.uint16)
    boxes, doms = [], []
    for j, name in enumerate(SPECIALS):
        ns, win, dom = special_window(name, T)
        assert ns == 17
        left = 1 + j * (T + 1)
        lab[1:1 + T, left:left + T] = win
        boxes.append((1, 1 + T, left, left + T))
        doms.append(dom)
    return lab, boxes, 17, np.array(doms, np.uint16)
