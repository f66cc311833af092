"""YCbCr frames shared by tests/test_yuv_views.py (host twin) and
tests/test_gpu_yuv_views.py (conversion kernel): the conversion of
include/photohive_dsp.h (phd_yuv_view) restated in numpy from its text --
chroma by replication or the triangle weights, then the 16.16 integer matrix
-- and every layout of the descriptor's table as offsets and byte strides
over one buffer of random bytes."""
import numpy as np

# (matrix, range) -> cy, crv, cgu, cgv, cbu, yoff
TABLE = {
    (0, 0): (65536, 91881, 22554, 46802, 116130, 0),       # BT601 FULL (JFIF)
    (0, 1): (76309, 104597, 25675, 53279, 132201, 16),     # BT601 LIMITED
    (1, 0): (65536, 103206, 12276, 30679, 121609, 0),      # BT709 FULL
    (1, 1): (76309, 117489, 13975, 34925, 138438, 16),     # BT709 LIMITED
}
# luma weights of the two matrices, for the real-valued conversion
KR_KB = {0: (0.299, 0.114), 1: (0.2126, 0.0722)}
# (matrix, range, chroma mode): both chroma modes over all four table rows
MODES = [(m, r, c) for c in (0, 1) for m in (0, 1) for r in (0, 1)]

SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 7), (17, 67), (33, 129), (9, 515)]
OFFSETS = (0, 1, 2, 3)
PITCH_EXTRA = (0, 1, 4)


def upsample(c, h, w, sx, sy, triangle):
    """Step 1: the chroma plane c [ch, cw] at every pixel of an h x w frame (int32)."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    ys, xs = np.arange(h), np.arange(w)
    if not triangle or sx == 0:
        return c[np.ix_(ys >> sy, xs >> sx)]
    i = xs >> 1
    far = np.clip(np.where(xs & 1, i + 1, i - 1), 0, cw - 1)
    if sy == 0:
        return (3 * c[:, i] + c[:, far] + np.where(xs & 1, 2, 1)) >> 2
    j = ys >> 1
    farrow = np.clip(np.where(ys & 1, j + 1, j - 1), 0, ch - 1)
    t = 3 * c[j, :] + c[farrow, :]
    return (3 * t[:, i] + t[:, far] + np.where(xs & 1, 7, 8)) >> 4


def matrix_rgb(Y, Cb, Cr, matrix, rng):
    """Step 2 on int32 arrays of one shape: [..., 3] uint8."""
    cy, crv, cgu, cgv, cbu, yoff = TABLE[(matrix, rng)]
    u, v = Cb.astype(np.int32) - 128, Cr.astype(np.int32) - 128
    yy = cy * (Y.astype(np.int32) - yoff)
    r = (yy + crv * v + 32768) >> 16
    g = (yy - cgu * u - cgv * v + 32768) >> 16
    b = (yy + cbu * u + 32768) >> 16
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def convert(Y, Cb, Cr, sx, sy, matrix, rng, chroma):
    """The packed RGB8 image [h, w, 3] the definition gives for the three planes."""
    h, w = Y.shape
    assert Cb.shape == Cr.shape == ((h + sy) >> sy, (w + sx) >> sx)
    return matrix_rgb(Y, upsample(Cb, h, w, sx, sy, chroma), upsample(Cr, h, w, sx, sy, chroma), matrix, rng)


def real_rgb(Y, Cb, Cr, matrix, rng):
    """The clamped real-valued matrix (float64), [..., 3]."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    sy_, sc, yoff = (255.0 / 219.0, 255.0 / 224.0, 16.0) if rng else (1.0, 1.0, 0.0)
    y = sy_ * (Y.astype(np.float64) - yoff)
    u, v = sc * (Cb.astype(np.float64) - 128.0), sc * (Cr.astype(np.float64) - 128.0)
    r = y + 2.0 * (1.0 - kr) * v
    b = y + 2.0 * (1.0 - kb) * u
    g = y - (kb * 2.0 * (1.0 - kb) / kg) * u - (kr * 2.0 * (1.0 - kr) / kg) * v
    return np.clip(np.stack([r, g, b], axis=-1), 0.0, 255.0)


# ---- layouts ---------------------------------------------------------------------
# name -> f(h, w, e) = dict(size, y, cb, cr, yrs, yps, crs, cps, sx, sy): the
# buffer's byte count and the offsets of the three (0,0) samples in it; e widens
# every pitch beyond its minimum.

def _cdims(h, w, sx, sy):
    return (h + sy) >> sy, (w + sx) >> sx


def _planar(sx, sy, swap=False, flip=False):
    def f(h, w, e):
        ch, cw = _cdims(h, w, sx, sy)
        yp, cp = w + e, cw + e
        y0, b0 = 0, h * yp + 1                       # (the planes one and two bytes apart from flush)
        r0 = b0 + ch * cp + 2
        size = r0 + ch * cp
        if swap:
            b0, r0 = r0, b0
        d = dict(size=size, y=y0, cb=b0, cr=r0, yrs=yp, yps=1, crs=cp, cps=1, sx=sx, sy=sy)
        if flip:                                     # rows bottom-up
            d.update(y=y0 + (h - 1) * yp, cb=b0 + (ch - 1) * cp, cr=r0 + (ch - 1) * cp, yrs=-yp, crs=-cp)
        return d
    return f


def _semi(swap, pitched=False, roi=False):
    def f(h, w, e):
        fh, fw, oy, ox = (h + 8, w + 10, 4, 6) if roi else (h, w, 0, 0)      # an even origin in a larger frame
        fch, fcw = _cdims(fh, fw, 1, 1)
        pitch = max(fw, 2 * fcw) + e + (5 if pitched else 0)
        uv0 = fh * pitch                             # the decoder surface: luma rows, then Cb Cr rows
        c0 = uv0 + (oy >> 1) * pitch + (ox >> 1) * 2
        return dict(size=uv0 + fch * pitch, y=oy * pitch + ox, cb=c0 + (1 if swap else 0),
                    cr=c0 + (0 if swap else 1), yrs=pitch, yps=1, crs=pitch, cps=2, sx=1, sy=1)
    return f


def _packed422(oy, ob, oc):
    def f(h, w, e):
        cw = (w + 1) >> 1
        pitch = 4 * cw + e
        return dict(size=h * pitch, y=oy, cb=ob, cr=oc, yrs=pitch, yps=2, crs=pitch, cps=4, sx=1, sy=0)
    return f


LAYOUTS = {
    "i420": _planar(1, 1),
    "yv12": _planar(1, 1, swap=True),
    "nv12": _semi(False),
    "nv21": _semi(True),
    "i422": _planar(1, 0),
    "i444": _planar(0, 0),
    "yuy2": _packed422(0, 1, 3),
    "uyvy": _packed422(1, 0, 2),
    "nv12_pitched": _semi(False, pitched=True),
    "nv12_roi": _semi(False, roi=True),
    "i420_flipped": _planar(1, 1, flip=True),
}


def plane(buf, at, shape, rs, ps):
    """The strided plane whose (0,0) sample is buf[at] (a copy)."""
    v = np.lib.stride_tricks.as_strided(buf[at:], shape=shape, strides=(rs, ps), writeable=False)
    return np.ascontiguousarray(v)


def yuv_case(name, h, w, off, extra, seed=0):
    """(buf, lay, (Y, Cb, Cr)): buf is off + size random bytes, lay the layout's
    dict with its three offsets moved by off, the planes numpy reads from it."""
    lay = dict(LAYOUTS[name](h, w, extra))
    rng = np.random.default_rng(seed * 1000003 + h * 131 + w * 7 + off * 3 + extra)
    buf = rng.integers(0, 256, off + lay["size"], dtype=np.uint8)
    for k in ("y", "cb", "cr"):
        lay[k] += off
    cshape = _cdims(h, w, lay["sx"], lay["sy"])
    planes = (plane(buf, lay["y"], (h, w), lay["yrs"], lay["yps"]),
              plane(buf, lay["cb"], cshape, lay["crs"], lay["cps"]),
              plane(buf, lay["cr"], cshape, lay["crs"], lay["cps"]))
    return buf, lay, planes


def make_view(base, lay, h, w, mode):
    """The PhdYuvView of a case whose buffer starts at address base."""
    from photohive_dsp_amd.structures import PhdYuvView
    m, r, c = mode
    return PhdYuvView(base + lay["y"], base + lay["cb"], base + lay["cr"], h, w, lay["yrs"], lay["yps"],
                      lay["crs"], lay["cps"], lay["sx"], lay["sy"], m, r, c)


def cube_planes():
    """All 256^3 (Y, Cb, Cr) triples as three 4096 x 4096 planes of a 4:4:4 frame."""
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return ((idx & 255).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx >> 16).astype(np.uint8))
