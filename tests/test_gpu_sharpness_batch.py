"""Per-image crop boxes in the batch entry points and the batched sharpness
kernel (sharpness.hip: k_sharp_tiles + k_sharp_finish) on the MI355X, against
oracle.sharpness (the C restatement, pinned bit-exact to the reference by the
structured_crops_600x800 fixture).  Both bars hold: FLOAT_RTOL = 1e-4 (the
contract) and TIGHT_RTOL = 1e-9 (tracked); a numpy restatement of the
tile-merge scheme measured 3.8e-14 at worst on these kinds and boxes."""
import ctypes

import numpy as np
import pytest

from tests.sharp_boxes import KINDS, assert_sharp, box, three, twelve
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu


def _images(h, w, n, seed0=40):
    from photohive_dsp_amd import synth
    return [synth.make(KINDS[i % len(KINDS)], h, w, seed0 + i) for i in range(n)]


def _sharp_ptr(rep):
    return rep.data_ptr.contents.sharpness


def _check_against_oracle(rep, img, boxes):
    """values, N and NULL-ness of one report's Sharpnesses"""
    from oracle import oracle as orc
    p = _sharp_ptr(rep)
    if boxes is None:
        assert not p and rep.sharpnesses == []
        return
    assert p and p.contents.N == len(boxes)
    assert len(rep.sharpnesses) == len(boxes)
    if boxes:
        assert_sharp(rep.sharpnesses, orc.sharpness(img, boxes))


def _same_other_fields(a, b):
    assert a.color_palette.group_ids == b.color_palette.group_ids
    assert a.color_palette.quantities == b.color_palette.quantities
    np.testing.assert_allclose(np.array(a.blur_profile.bins), np.array(b.blur_profile.bins), rtol=1e-12, atol=1e-15)
    assert [(v.angle, v.magnitude) for v in a.blur_vectors] == [(v.angle, v.magnitude) for v in b.blur_vectors]
    sa, sb = a.rgb_stats, b.rgb_stats
    assert [sa.Br, sa.Bg, sa.Bb, sa.Cr, sa.Cg, sa.Cb] == [sb.Br, sb.Bg, sb.Bb, sb.Cr, sb.Cg, sb.Cb]
    np.testing.assert_allclose(a.average_saturation, b.average_saturation, rtol=1e-12)


@pytest.mark.parametrize("h,w", [(480, 640), (513, 700), (401, 577)])
def test_batch_boxes_against_oracle(h, w):
    """Compile-time batched FFT path, runtime-plan batched path, odd size: five
    images with twelve boxes / None / [] / the whole image / three boxes."""
    phd, L, torch = _phd()
    imgs = _images(h, w, 5)
    lists = [twelve(h, w), None, [], [box(0, h, 0, w)], three(h, w)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    with_boxes = phd.report_device(t, salient_characters=lists)
    plain = phd.report_device(t)
    for rep, ref, img, boxes in zip(with_boxes, plain, imgs, lists):
        _check_against_oracle(rep, img, boxes)
        _same_other_fields(rep, ref)
        assert not _sharp_ptr(ref)
    # the duplicate box: the same bits
    assert with_boxes[0].sharpnesses[6] == with_boxes[0].sharpnesses[7]
    # more boxes than to_json's ten: the first ten are written
    assert '"Sharpness 10:"' in with_boxes[0].to_json()


def test_box_value_is_a_pure_function_of_image_and_box():
    """One image and its twelve boxes alone, at index 3 of 5, at index 16 of 17
    on two lanes and on one, three times each: every list compares ==, and
    sharpness_device gives the report's bits."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import sharpness_device
    h, w = 480, 640
    imgs = _images(h, w, 17, seed0=70)
    target = imgs[5]
    boxes = twelve(h, w)
    other = three(h, w)

    def run(n, at):
        stack = [imgs[(k + 1) % 17] for k in range(n)]
        stack[at] = target
        lists = [other if k % 2 else None for k in range(n)]
        lists[at] = boxes
        t = torch.from_numpy(np.stack(stack)).cuda()
        reps = phd.report_device(t, salient_characters=lists)
        alone = sharpness_device(t, lists)
        assert alone[at] == reps[at].sharpnesses
        return reps[at].sharpnesses

    seen = []
    prev = L.lib.phd_set_lanes(0)
    try:
        for _ in range(3):
            seen.append(run(1, 0))
            seen.append(run(5, 3))
            L.lib.phd_set_lanes(2)
            seen.append(run(17, 16))
            L.lib.phd_set_lanes(1)
            seen.append(run(17, 16))
            L.lib.phd_set_lanes(prev)
    finally:
        L.lib.phd_set_lanes(prev)
    assert len(seen[0]) == 12
    for s in seen[1:]:
        assert s == seen[0]


def test_two_lanes_each_image_its_own_boxes():
    """17 images at 480 x 640 on two lanes (9 + 8), a different box list per
    image: a lane reading the wrong part of the table shows."""
    phd, L, torch = _phd()
    h, w = 480, 640
    imgs = _images(h, w, 17, seed0=90)
    pool = twelve(h, w) + three(h, w)
    lists = []
    for i in range(17):
        if i % 6 == 4:
            lists.append(None)
        else:
            lists.append([pool[(i + 3 * k) % len(pool)] for k in range(1 + i % 4)] +
                         [box(i, 100 + 7 * i, 2 * i, 300 + i)])
    t = torch.from_numpy(np.stack(imgs)).cuda()
    prev = L.lib.phd_set_lanes(2)
    try:
        reps = phd.report_device(t, salient_characters=lists)
    finally:
        L.lib.phd_set_lanes(prev)
    for rep, img, boxes in zip(reps, imgs, lists):
        _check_against_oracle(rep, img, boxes)


def _mixed_inputs():
    sizes = [(512, 512), (480, 640), (512, 512)]
    from photohive_dsp_amd import synth
    imgs = [synth.make(KINDS[i], h, w, 120 + i) for i, (h, w) in enumerate(sizes)]
    lists = [three(512, 512), twelve(480, 640), [box(0, 512, 0, 512), box(500, 512, 1, 512)]]
    return imgs, lists


def test_mixed_sizes_device_and_host():
    phd, L, torch = _phd()
    imgs, lists = _mixed_inputs()
    dev = phd.reports_device_mixed([torch.from_numpy(i).cuda() for i in imgs], salient_characters=lists)
    host = phd.get_reports(imgs, salient_characters=lists)
    for reps in (dev, host):
        for rep, img, boxes in zip(reps, imgs, lists):
            _check_against_oracle(rep, img, boxes)
    for a, b in zip(dev, host):
        assert a.sharpnesses == b.sharpnesses


def test_mixed_sizes_a_rejected_size_fails_alone():
    phd, L, torch = _phd()
    imgs, lists = _mixed_inputs()
    imgs.insert(1, np.full((349, 350, 3), 90, np.uint8))
    lists.insert(1, [box(0, 10, 0, 10)])
    reps = phd.get_reports(imgs, salient_characters=lists)
    assert reps[1] is None
    for k in (0, 2, 3):
        _check_against_oracle(reps[k], imgs[k], lists[k])


def test_mixed_sizes_a_bad_box_fails_alone():
    """right = width + 1 on one image: that image alone is NULL with status < 0
    and the message names it; host and device entry points."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import make_config, normalize_salient
    from photohive_dsp_amd.structures import Full_Report_Data
    imgs, lists = _mixed_inputs()
    lists[1] = lists[1][:3] + [box(0, 10, 0, 641)]
    reps = phd.get_reports(imgs, salient_characters=lists)
    assert reps[1] is None
    assert "image 1" in L.last_error() and "crop 3" in L.last_error()
    for k in (0, 2):
        _check_against_oracle(reps[k], imgs[k], lists[k])
    # the device call, through the C-ABI
    n = 3
    ts = [torch.from_numpy(i).cuda() for i in imgs]
    crops = normalize_salient(lists, n)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    hs = (ctypes.c_int * n)(*[t.shape[0] for t in ts])
    ws = (ctypes.c_int * n)(*[t.shape[1] for t in ts])
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    cfg = make_config()
    torch.cuda.synchronize()
    rc = L.lib.phd_report_batch_device_mixed_crops(ptrs, hs, ws, n, ctypes.byref(cfg), crops[0], outs, st, None)
    assert rc == 1 and st[1] < 0 and not outs[1] and st[0] == 0 and st[2] == 0
    assert "image 1" in L.last_error()
    from photohive_dsp_amd.core import _finish
    for k in (0, 2):
        _check_against_oracle(_finish(outs[k], hs[k], ws[k], {}), imgs[k], lists[k])


def test_downsampled_report_keeps_full_resolution_boxes():
    """downsample_rate = 2 shrinks the palette's image only; the sharpness is
    of the full-resolution luma (src/interface.c:50,73)."""
    phd, L, torch = _phd()
    h, w = 600, 800
    imgs = _images(h, w, 2, seed0=150)
    lists = [twelve(h, w), three(h, w)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    reps = phd.report_device(t, salient_characters=lists, downsample_rate=2)
    for rep, img, boxes in zip(reps, imgs, lists):
        _check_against_oracle(rep, img, boxes)


def test_image_stride_with_padding():
    """The raw C calls with image_stride > 3 h w and the padding filled with
    255: boxes flush with the last row read nothing of it."""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd.core import _finish, make_config, normalize_salient
    from photohive_dsp_amd.structures import Full_Report_Data
    h, w, n = 401, 577, 3
    imgs = _images(h, w, n, seed0=170)
    stride = 3 * h * w + 1021
    buf = np.full((n, stride), 255, np.uint8)
    for i, im in enumerate(imgs):
        buf[i, :3 * h * w] = im.reshape(-1)
    t = torch.from_numpy(buf).cuda()
    lists = [twelve(h, w), [box(h - 1, h, 0, w), box(h - 17, h, w - 65, w)], [box(0, h, 0, w)]]
    crops = normalize_salient(lists, n)
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    cfg = make_config()
    torch.cuda.synchronize()
    rc = L.lib.phd_report_batch_device_crops(t.data_ptr(), n, h, w, stride, ctypes.byref(cfg), crops[0], outs, st,
                                             None)
    assert rc == 0, L.last_error()
    reps = [_finish(outs[i], h, w, {}) for i in range(n)]
    for rep, img, boxes in zip(reps, imgs, lists):
        _check_against_oracle(rep, img, boxes)
    flat = (ctypes.c_double * sum(len(b) for b in lists))()
    assert L.lib.phd_sharpness_batch_device(t.data_ptr(), n, h, w, stride, crops[0], flat, None) == 0
    assert list(flat) == [v for rep in reps for v in rep.sharpnesses]
    assert_sharp(list(flat), np.concatenate([orc.sharpness(im, b) for im, b in zip(imgs, lists)]))


def test_full_size_two_images_ten_boxes():
    phd, L, torch = _phd()
    h, w = 3000, 4000
    t = torch.empty((2, h, w, 3), dtype=torch.uint8, device="cuda")
    assert L.lib.phd_fill_structured_device(t[0].data_ptr(), h, w, 201, 0, 1, None) == 0
    assert L.lib.phd_fill_uniform_device(t[1].data_ptr(), h * w * 3, 202, None) == 0
    torch.cuda.synchronize()
    imgs = list(t.cpu().numpy())
    ten = [box(0, h, 0, w)] + [box(300 * k, 300 * k + 500, 400 * k, 400 * k + 500) for k in range(8)] + \
          [box(h - 500, h, w - 500, w)]
    reps = phd.report_device(t, salient_characters=[ten, ten])
    for rep, img in zip(reps, imgs):
        _check_against_oracle(rep, img, ten)


def test_sharpness_launches_are_profiled():
    """kSharp brackets: two launches per batched call (tiles + finish), two per
    box on the single-image path."""
    phd, L, torch = _phd()
    h, w = 480, 640
    imgs = _images(h, w, 2, seed0=190)
    t = torch.from_numpy(np.stack(imgs)).cuda()
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    L.lib.phd_profile_kernels(1 << 5)
    try:
        phd.report_device(t, salient_characters=[three(h, w), twelve(h, w)])
        L.lib.phd_profile_read(5, ctypes.byref(tot), ctypes.byref(cnt))
        assert cnt.value == 2 and tot.value > 0
        phd.get_report(imgs[0], salient_characters=phd.set_bounding_boxes(three(h, w)))
        L.lib.phd_profile_read(5, ctypes.byref(tot), ctypes.byref(cnt))
        assert cnt.value == 2 + 6
    finally:
        L.lib.phd_profile_kernels(0)
