"""CPU tests of the labels from depth maps (kfnet_amd/labels.py): the two restatements of tests/labels_ref.py on
cases known by hand and against each other within the derived bound, the 16-bit PNG decoder (host code of the built
library), the decorrelating transform, the descriptor's constants, read_sequence, the command lines' refusals, the new
exports' argument checks (no device needed: nothing is launched) and the ABI number."""
import ctypes as C
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import labels_ref as R
from kfnet_amd import _lib
from kfnet_amd import labels as L
from kfnet_amd.labels import DepthCamera, decorrelating_transform, load_depth, read_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = DepthCamera(525., 525., 320., 240.)
# 7-Scenes' depth camera as commonly calibrated: focal length 585, same principal point
CAM_REG = DepthCamera(525., 525., 320., 240., depth_fx=585., depth_fy=585.)
IDENTITY = np.eye(4)[None]


# -- 1. the restatements on cases known by hand ----------------------------------------------------------------------------
def _one_pixel(H, W, y, x, raw):
    d = np.zeros((1, H, W), np.uint16)
    d[0, y, x] = raw
    return d


@pytest.mark.parametrize('fn', [R.labels32, R.labels64])
def test_principal_point_at_one_metre_under_the_identity_pose(fn):
    cam = DepthCamera(525., 525., 16., 8.)
    out = fn(_one_pixel(16, 32, 8, 16, 1000), IDENTITY, cam, 1)
    if fn is R.labels32:
        assert out.dtype == np.float32
        assert np.array_equal(out[0, 8, 16], np.float32([0, 0, np.float32(1000) * np.float32(0.001), 1]))
        assert np.array_equal(out[0, 8, 16], np.float32([0, 0, 1, 1]))       # 1000 * f32(0.001) = 1 + 4.7e-8 rounds to 1
    else:
        assert np.allclose(out[0, 8, 16], [0, 0, 1, 1], rtol=0, atol=1e-15)
    assert out[..., 3].sum() == 1 and np.all(out[0, 0, 0] == 0)
    # stride 8 reads colour pixel (8c, 8r): cell (1, 2) is pixel x = 16, y = 8
    grid = fn(_one_pixel(16, 32, 8, 16, 1000), IDENTITY, cam, 8)
    assert grid.shape == (1, 2, 4, 4) and np.array_equal(grid[0, 1, 2], out[0, 8, 16]) and grid[..., 3].sum() == 1


@pytest.mark.parametrize('fn', [R.labels32, R.labels64])
def test_raw_0_and_65535_give_four_zeros(fn):
    d = np.full((1, 8, 8), 1000, np.uint16)
    d[0, 2, 3], d[0, 5, 6] = 0, 65535
    out = fn(d, IDENTITY, CAM, 1)
    assert np.all(out[0, 2, 3] == 0) and np.all(out[0, 5, 6] == 0)
    assert out[..., 3].sum() == 62 and np.all(out[0, 2, 4, 3] == 1)
    # the window's ends themselves are valid
    d[0, 2, 3], d[0, 5, 6] = 1, 65534
    assert fn(d, IDENTITY, CAM, 1)[..., 3].sum() == 64


@pytest.mark.parametrize('fn', [R.labels32, R.labels64])
def test_a_ninety_degree_pose(fn):
    """Camera-to-world R = rotation by +90 degrees about z (x -> y, y -> -x) with centre (1, 2, 3): the camera point
    (X, Y, z) lands at (1 - Y, 2 + X, 3 + z).  Depth is z, not ray length: pixel (x, y) = (u + 105, v + 210) at raw 2000 is
    (0.4, 0.8, 2.0)."""
    cam = DepthCamera(525., 525., 20., 10.)
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    out = fn(_one_pixel(224, 128, 220, 125, 2000), T[None], cam, 1)
    tol = 1e-6 if fn is R.labels32 else 1e-12
    assert np.allclose(out[0, 220, 125], [1 - 0.8, 2 + 0.4, 3 + 2.0, 1], rtol=0, atol=tol)


def test_registration_moves_pixel_zero_to_the_expected_depth_column():
    """depth_fx = 585 against fx = 525, both principal points at 320: colour column 0 reads depth column
    round(-320 * 585 / 525 + 320) = round(-36.571) = -37, outside; the first column inside is the first x with
    (x - 320) * 585 / 525 + 320 >= -0.5, x = 33 (-0.2), and colour column 320 reads depth column 320."""
    for dtype in (np.float32, np.float64):
        x, y, xd, yd, ok_x, ok_y = R.depth_pixels(CAM_REG, 480, 640, 1, dtype)
        assert not ok_x[0] and not ok_x[32] and ok_x[33] and xd[33] == 0 and xd[320] == 320
        # the last column inside: (606 - 320) * 585 / 525 + 320 = 638.69 -> 639; x = 607 gives 639.8 -> 640, outside
        assert xd[34] == 1 and ok_x[606] and xd[606] == 639 and not ok_x[607] and not ok_x[639]
        assert not ok_y[0] and yd[240] == 240
    d = np.zeros((1, 480, 640), np.uint16)
    d[0, 240, 0] = 1500                 # depth pixel (0, 240) is seen by colour pixel (33, 240)
    out = R.labels32(d, IDENTITY, CAM_REG, 1)
    assert out[..., 3].sum() == 1 and out[0, 240, 33, 3] == 1
    assert abs(out[0, 240, 33, 0] - (33 - 320) / 525 * 1.5) < 1e-6       # back-projected with the COLOUR pixel
    assert np.all(out[0, 240, 0] == 0)


def test_round_half_away_from_zero():
    t = np.float32([0.5, -0.5, 1.5, -1.5, 2.4999998, 0.49999997, -0.49999997, 7.0])
    assert np.array_equal(R.round_half_away(t), np.float32([1, -1, 2, -2, 2, 0, -0, 7]))


# -- 2. float32 against fp64, within the derived bound -----------------------------------------------------------------------
@pytest.mark.parametrize('cam', [CAM, CAM_REG], ids=['plain', 'registered'])
@pytest.mark.parametrize('stride', [1, 8])
def test_float32_restatement_stays_within_the_derived_bound_of_fp64(cam, stride):
    """Every pixel: none is left out.  The two agree on which depth pixel a colour pixel reads: (x - 320) * 585 / 525 is
    never within 1/70 of a half (78 (x - 320) = 35 (2k + 1) has no solution: even against odd), four hundred times the fp32
    error of that expression."""
    rng = np.random.default_rng(5)
    B, H, W = 3, 480, 640
    depth = R.random_depth(rng, B, H, W)
    poses = np.stack([R.random_pose(rng) for _ in range(B)])
    for a, b in zip(R.depth_pixels(cam, H, W, stride, np.float32), R.depth_pixels(cam, H, W, stride, np.float64)):
        assert np.array_equal(a, b)
    a32, a64 = R.labels32(depth, poses, cam, stride), R.labels64(depth, poses, cam, stride)
    assert a32.shape == (B, H // stride, W // stride, 4)
    assert np.array_equal(a32[..., 3], a64[..., 3]) and 0.5 < a32[..., 3].mean() < 0.8
    err = np.abs(a32[..., :3].astype(np.float64) - a64[..., :3])
    lim = R.bound(depth, poses, cam, stride)
    print('largest error / bound: %.3f' % float((err / np.maximum(lim, 1e-300))[a64[..., 3] == 1].max()))
    assert np.all(err <= lim)
    assert np.all(a32[a32[..., 3] == 0] == 0)


# -- 3. the 16-bit PNG decoder ----------------------------------------------------------------------------------------------
H16, W16 = 11, 13


def _decode16(paths, size=(H16, W16), fill=12345, threads=3):
    lib = _lib.load()
    n = len(paths)
    dst = np.full((n, size[0], size[1]), fill, np.uint16)
    arr = (C.c_char_p * n)(*[os.fsencode(str(p)) for p in paths])
    status = (C.c_int * n)()
    rc = lib.kfn_decode_png_gray16(arr, n, size[0], size[1], dst.ctypes.data, status, threads)
    return rc, list(status), dst, lib.kfn_last_error().decode()


def _samples(seed):
    a = np.random.default_rng(seed).integers(0, 65536, size=(H16, W16)).astype(np.uint16)
    a[0, :5] = [0, 1, 255, 256, 65535]          # low byte only, high byte only, both ends
    a[H16 - 1, -5:] = [65535, 256, 255, 1, 0]
    return a


@pytest.mark.parametrize('first', range(5))
@pytest.mark.parametrize('pieces', [1, 4])
def test_gray16_every_filter_type_and_idat_split(tmp_path, first, pieces):
    """Rows cycle through the filters starting at `first` (each is once the first row, which has no row above)."""
    a = _samples(first)
    p = tmp_path / 'd.png'
    R.write_png16(p, a, filters=[(first + y) % 5 for y in range(H16)], idat_pieces=pieces)
    rc, status, dst, _ = _decode16([p])
    assert rc == 0 and status == [_lib.PNG_OK]
    assert np.array_equal(dst[0], a)
    assert np.array_equal(load_depth([str(p)], (H16, W16)), a[None])


def test_gray16_agrees_with_pil_and_reads_what_pil_writes(tmp_path):
    from PIL import Image
    a = _samples(9)
    p, q = tmp_path / 'ours.png', tmp_path / 'pil.png'
    R.write_png16(p, a, filters=[4] * H16)
    Image.fromarray(a).save(q)
    with Image.open(p) as im:
        assert np.array_equal(np.asarray(im).astype(np.uint16), a)
    rc, status, dst, _ = _decode16([p, q])
    assert rc == 0 and status == [_lib.PNG_OK] * 2 and np.array_equal(dst[0], a) and np.array_equal(dst[1], a)


def _other_kinds(tmp_path):
    rng = np.random.default_rng(1)
    g8 = rng.integers(0, 256, size=(H16, W16), dtype=np.uint8)
    rgb16 = rng.integers(0, 65536, size=(H16, W16 * 3)).astype('>u2')
    g16 = rng.integers(0, 65536, size=(H16, W16)).astype('>u2')
    files = {
        'gray8.png': R.png_bytes([g8[y].tobytes() for y in range(H16)], W16, 0, 8, [0] * H16),
        'rgb16.png': R.png_bytes([rgb16[y].tobytes() for y in range(H16)], W16, 2, 16, [0] * H16),
        # (the Adam7 flag alone: the decoder must refuse before it looks at the data)
        'interlaced.png': R.png_bytes([g16[y].tobytes() for y in range(H16)], W16, 0, 16, [0] * H16, interlace=1),
        'not_a_png.png': b'\xff\xd8\xff\xe0' + bytes(100),
    }
    paths = []
    for name, data in files.items():
        with open(tmp_path / name, 'wb') as f:
            f.write(data)
        paths.append(tmp_path / name)
    return paths


def test_gray16_other_kinds_are_unsupported_and_leave_dst_untouched(tmp_path):
    good = tmp_path / 'good.png'
    R.write_png16(good, _samples(2))
    paths = _other_kinds(tmp_path) + [good]
    rc, status, dst, _ = _decode16(paths)
    assert rc == 0
    assert status == [_lib.PNG_UNSUPPORTED] * 4 + [_lib.PNG_OK]
    assert np.all(dst[:4] == 12345) and np.array_equal(dst[4], _samples(2))


def test_load_depth_hands_unsupported_files_to_pil(tmp_path):
    from PIL import Image
    a = np.random.default_rng(3).integers(0, 256, size=(H16, W16), dtype=np.uint8)
    p = tmp_path / 'gray8.png'
    Image.fromarray(a).save(p)
    assert np.array_equal(load_depth([str(p)], (H16, W16)), a[None].astype(np.uint16))
    rgb = tmp_path / 'rgb.png'
    Image.fromarray(np.zeros((H16, W16, 3), np.uint8)).save(rgb)
    with pytest.raises(ValueError, match='rgb.png'):
        load_depth([str(rgb)], (H16, W16))


def _broken(tmp_path):
    a = _samples(4)
    good = R.png_bytes([a[y].astype('>u2').tobytes() for y in range(H16)], W16, 0, 16, [1] * H16)
    idat = good.index(b'IDAT')
    bad_crc = bytearray(good)
    bad_crc[idat + 10] ^= 0x40                       # a data byte of IDAT: its CRC no longer matches
    raw = b''.join(b'\x00' + a[y].astype('>u2').tobytes() for y in range(H16))
    z = bytearray(zlib.compress(raw, 0))             # stored blocks: a flipped payload byte breaks only adler32
    z[20] ^= 0x01
    bad_zlib = (good[:8] + R.chunk(b'IHDR', struct.pack('>IIBBBBB', W16, H16, 16, 0, 0, 0, 0)) + R.chunk(b'IDAT', bytes(z)) +
                R.chunk(b'IEND', b''))
    short = zlib.compress(raw[:len(raw) // 2], 6)
    half = (good[:8] + R.chunk(b'IHDR', struct.pack('>IIBBBBB', W16, H16, 16, 0, 0, 0, 0)) + R.chunk(b'IDAT', short) +
            R.chunk(b'IEND', b''))
    files = {'truncated.png': good[:len(good) // 2], 'bad_crc.png': bytes(bad_crc), 'bad_zlib.png': bad_zlib,
             'half_the_rows.png': half,
             'wrong_size.png': R.png_bytes([a[y, :W16 - 1].astype('>u2').tobytes() for y in range(H16)], W16 - 1, 0, 16, [0] * H16)}
    out = {}
    for name, data in files.items():
        with open(tmp_path / name, 'wb') as f:
            f.write(data)
        out[name] = tmp_path / name
    out['missing.png'] = tmp_path / 'missing.png'
    return out


@pytest.mark.parametrize('name', ['truncated.png', 'bad_crc.png', 'bad_zlib.png', 'half_the_rows.png', 'wrong_size.png',
                                  'missing.png'])
def test_gray16_broken_files_are_errors_that_name_the_file(tmp_path, name):
    good = tmp_path / 'good.png'
    R.write_png16(good, _samples(2))
    bad = _broken(tmp_path)[name]
    rc, status, dst, msg = _decode16([good, bad, good])
    assert rc == -1                                                  # KFN_ERR_ARG
    assert status == [_lib.PNG_OK, _lib.PNG_ERROR, _lib.PNG_OK]
    assert name in msg and 'kfn_decode_png_gray16' in msg
    assert np.all(dst[1] == 12345) and np.array_equal(dst[0], _samples(2))
    with pytest.raises(ValueError, match=name):
        load_depth([str(good), str(bad)], (H16, W16))


def test_rgb8_decoder_still_reports_16_bit_files_as_unsupported(tmp_path):
    p = tmp_path / 'd.png'
    R.write_png16(p, _samples(6))
    lib = _lib.load()
    dst = np.full((1, H16, W16, 3), 77, np.uint8)
    status = (C.c_int * 1)()
    arr = (C.c_char_p * 1)(os.fsencode(str(p)))
    assert lib.kfn_decode_png_rgb8(arr, 1, H16, W16, dst.ctypes.data, status, 1) == 0
    assert status[0] == _lib.PNG_UNSUPPORTED and np.all(dst == 77)


def test_gray16_argument_checks():
    lib = _lib.load()
    assert lib.kfn_decode_png_gray16(None, 0, 8, 8, None, None, 1) == 0
    assert lib.kfn_decode_png_gray16(None, 1, 8, 8, None, None, 1) == -1
    arr = (C.c_char_p * 1)(b'x.png')
    dst = np.zeros((1, 8, 8), np.uint16)
    assert lib.kfn_decode_png_gray16(arr, 1, 0, 8, dst.ctypes.data, None, 1) == -1


# -- 4. the decorrelating transform ------------------------------------------------------------------------------------------
def _cloud(n=20000, seed=0):
    """An anisotropic cloud with known rotation and mean: sigma (3, 1, 0.2) along the rows of a random rotation."""
    rng = np.random.default_rng(seed)
    Q = R.random_pose(rng)[:3, :3]
    mean = np.array([4.0, -7.0, 2.5])
    p = (rng.normal(size=(n, 3)) * [3.0, 1.0, 0.2]).dot(Q) + mean
    return p, Q, mean


def _moments_of(p, pivot):
    d = p - pivot
    return np.concatenate([[len(p)], d.sum(0), [(d[:, i] * d[:, j]).sum() for i in range(3) for j in range(i, 3)]])


def test_transform_decorrelates_to_fp64_precision():
    p, Q, mean = _cloud()
    pivot = p[0] + [0.5, -0.3, 0.2]
    M = decorrelating_transform(_moments_of(p, pivot), pivot)
    assert M.dtype == np.float64 and np.array_equal(M[3], [0, 0, 0, 1])
    q = p.dot(M[:3, :3].T) + M[:3, 3]
    cov_p = np.cov(p.T, bias=True)
    tr = np.trace(cov_p)
    cov_q = np.cov(q.T, bias=True)
    off = np.abs(cov_q - np.diag(np.diag(cov_q))).max()
    print('|mean| %.3g, off-diagonal %.3g, limit %.3g' % (np.abs(q.mean(0)).max(), off, 1e-9 * tr))
    assert np.abs(q.mean(0)).max() < 1e-9 * tr
    assert off < 1e-9 * tr
    Rm = M[:3, :3]
    assert np.abs(Rm.dot(Rm.T) - np.eye(3)).max() < 1e-9
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-9 and np.linalg.det(Rm) > 0
    # descending variances, the cloud's own axes (up to sign) and mean
    assert cov_q[0, 0] > cov_q[1, 1] > cov_q[2, 2]
    assert np.allclose(np.diag(cov_q), np.sort(np.linalg.eigvalsh(cov_p))[::-1], rtol=1e-9)
    assert np.allclose(np.abs(Rm.dot(Q.T)), np.eye(3), atol=0.05)
    assert np.allclose(-Rm.T.dot(M[:3, 3]), p.mean(0), rtol=0, atol=1e-9)


def test_transform_sign_and_handedness_conventions():
    """Rows 0 and 1: the largest-magnitude component is positive.  Row 2 takes the sign that makes det R = +1, so its own
    largest component is positive only when that agrees with a right-handed frame."""
    for seed in range(8):
        p, _, _ = _cloud(2000, seed)
        M = decorrelating_transform(_moments_of(p, p[0]), p[0])
        Rm = M[:3, :3]
        for i in (0, 1):
            assert Rm[i, np.argmax(np.abs(Rm[i]))] > 0
        assert np.linalg.det(Rm) > 0.999999
        assert np.allclose(np.cross(Rm[0], Rm[1]), Rm[2], atol=1e-12)
    # an axis-aligned cloud: variances (1, 9, 4) along (x, y, z) -> rows y, z, x: an even permutation, no flip
    rng = np.random.default_rng(0)
    p = rng.normal(size=(50000, 3)) * [1.0, 3.0, 2.0]
    M = decorrelating_transform(_moments_of(p, np.zeros(3)), np.zeros(3))
    assert np.allclose(M[:3, :3], [[0, 1, 0], [0, 0, 1], [1, 0, 0]], atol=0.05)
    # variances (9, 1, 4): rows x, z, y would be left-handed, so the third row comes out as -y
    p = rng.normal(size=(50000, 3)) * [3.0, 1.0, 2.0]
    M = decorrelating_transform(_moments_of(p, np.zeros(3)), np.zeros(3))
    assert np.allclose(M[:3, :3], [[1, 0, 0], [0, 0, 1], [0, -1, 0]], atol=0.05)


def test_transform_is_the_same_from_moments_about_two_pivots():
    p, _, mean = _cloud()
    a = decorrelating_transform(_moments_of(p, p[0]), p[0])
    b = decorrelating_transform(_moments_of(p, mean + [1.0, 2.0, -1.5]), mean + [1.0, 2.0, -1.5])
    scale = np.abs(a).max()
    assert np.abs(a - b).max() < 1e-9 * scale


def test_transform_needs_points_and_writes_nine_digits(tmp_path):
    with pytest.raises(ValueError):
        decorrelating_transform(np.zeros(10), np.zeros(3))
    p, _, _ = _cloud(500)
    M = decorrelating_transform(_moments_of(p, p[0]), p[0])
    L.write_transform(str(tmp_path / 'transform.txt'), M)
    back = np.loadtxt(str(tmp_path / 'transform.txt'))
    assert back.shape == (4, 4) and np.allclose(back, M, rtol=1e-9, atol=1e-9)
    assert np.array_equal(L.add_frames(None, np.arange(20.0).reshape(2, 10)), np.arange(10.0) * 2 + 10)


# -- 5. the descriptor's constants ---------------------------------------------------------------------------------------------
def _bits(x):
    return np.float32(x).view(np.uint32)


def test_descriptor_constants_are_the_fp64_expressions_rounded_once():
    cam = DepthCamera(525.3, 524.1, 319.7, 241.2, depth_fx=585.6, depth_fy=584.9, depth_u=322.4, depth_v=238.8, scale=0.001,
                      raw_min=2, raw_max=60000)
    d = cam.descriptor(3, 24, 40, 8, ld_out=6)
    assert (d.struct_size, d.B, d.H, d.W, d.stride, d.ld_out) == (C.sizeof(_lib.DepthLabelsDesc), 3, 24, 40, 8, 6)
    assert (d.registration, d.raw_min, d.raw_max) == (1, 2, 60000)
    want = dict(u=319.7, v=241.2, inv_fx=1.0 / 525.3, inv_fy=1.0 / 524.1, kx=585.6 / 525.3, ky=584.9 / 524.1, ud=322.4, vd=238.8,
                scale=0.001)
    for name, value in want.items():
        assert _bits(getattr(d, name)) == _bits(np.float32(value)), name
        assert _bits(getattr(d, name)) == _bits(R.constants(cam, np.float32)[name]), name
    # not the float32 quotient of float32 operands
    assert _bits(np.float32(585.6) / np.float32(525.3)) != _bits(d.kx) or _bits(np.float32(1) / np.float32(525.3)) != _bits(d.inv_fx) \
        or _bits(np.float32(584.9) / np.float32(524.1)) != _bits(d.ky)
    plain = DepthCamera().descriptor(1, 8, 8, 1)
    assert (plain.registration, plain.raw_min, plain.raw_max, plain.ld_out) == (0, 1, 65534, 4)
    assert (plain.u, plain.v, plain.kx, plain.ud) == (320.0, 240.0, 1.0, 320.0)
    assert _bits(plain.scale) == _bits(np.float32(0.001)) and _bits(plain.inv_fx) == _bits(np.float32(1.0 / 525.0))


def test_camera_refuses_impossible_values():
    for kw in (dict(fx=0.0), dict(depth_fy=-1.0), dict(raw_min=5, raw_max=4), dict(raw_max=70000)):
        with pytest.raises(ValueError):
            DepthCamera(**kw)
    assert np.array_equal(L.pose_rows(np.eye(4)[None]), np.float32([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]))
    with pytest.raises(ValueError):
        L.pose_rows(np.zeros((2, 5)))


# -- 6. read_sequence --------------------------------------------------------------------------------------------------------
def _touch_sequence(folder, indices):
    os.makedirs(str(folder), exist_ok=True)
    for i in indices:
        for ext in ('color.png', 'depth.png', 'pose.txt'):
            open(os.path.join(str(folder), 'frame-%06d.%s' % (i, ext)), 'w').close()


def test_read_sequence_sorts_and_pairs(tmp_path):
    _touch_sequence(tmp_path / 's', [10, 2, 0, 1])
    t = read_sequence(str(tmp_path / 's'))
    assert [os.path.basename(c) for c, _, _ in t] == ['frame-%06d.color.png' % i for i in (0, 1, 2, 10)]
    for c, d, p in t:
        assert d == c.replace('color.png', 'depth.png') and p == c.replace('color.png', 'pose.txt')


def test_read_sequence_names_what_is_missing(tmp_path):
    s = tmp_path / 's'
    _touch_sequence(s, range(3))
    os.remove(str(s / 'frame-000001.pose.txt'))
    with pytest.raises(ValueError, match='frame-000001.pose.txt'):
        read_sequence(str(s))
    _touch_sequence(s, range(3))
    open(str(s / 'frame-000007.depth.png'), 'w').close()          # a depth map without its colour image
    with pytest.raises(ValueError, match='3 colour images, 4 depth maps'):
        read_sequence(str(s))
    with pytest.raises(ValueError, match='empty'):
        os.makedirs(str(tmp_path / 'empty'))
        read_sequence(str(tmp_path / 'empty'))
    with pytest.raises(ValueError, match='nowhere'):
        read_sequence(str(tmp_path / 'nowhere'))


def test_read_sequence_takes_a_folder_of_lists(tmp_path):
    s = tmp_path / 's'
    _touch_sequence(s, range(3))
    t = read_sequence(str(s))
    lists = tmp_path / 'lists'
    os.makedirs(str(lists))
    for name, col in zip(L.LISTS, zip(*t)):
        with open(str(lists / name), 'w') as f:
            f.write(''.join(p + '\n' for p in col))
    assert read_sequence(str(lists)) == t
    with open(str(lists / 'pose_list.txt'), 'w') as f:
        f.write(''.join(p + '\n' for p in list(zip(*t))[2][:2]))
    with pytest.raises(ValueError, match='pose_list.txt lists 2 files for the 3 images'):
        read_sequence(str(lists))
    os.remove(str(lists / 'pose_list.txt'))
    with pytest.raises(ValueError, match='pose_list.txt is missing'):
        read_sequence(str(lists))
    with open(str(lists / 'pose_list.txt'), 'w') as f:
        f.write(''.join(p + '\n' for p in list(zip(*t))[2][:2]) + str(s / 'gone.pose.txt') + '\n')
    with pytest.raises(ValueError, match='gone.pose.txt is missing'):
        read_sequence(str(lists))


# -- 7. the command lines' refusals (no device is touched before they are checked) ---------------------------------------
def _run(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    return subprocess.run([sys.executable, '-m', module] + list(args), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)


def test_labels_make_argument_errors(tmp_path, capsys):
    s = tmp_path / 's'
    _touch_sequence(s, range(2))
    out = str(tmp_path / 'out')
    assert L.main(['make', '--output_folder', out]) == 1
    assert '--sequence' in capsys.readouterr().err
    assert L.main(['make', '--sequence', str(s)]) == 1
    assert '--output_folder' in capsys.readouterr().err
    assert L.main(['make', '--sequence', str(s), '--output_folder', out, '--height', '100']) == 1
    assert 'multiples of 8' in capsys.readouterr().err
    assert L.main(['make', '--sequence', str(s), '--output_folder', out, '--batch', '0']) == 1
    assert '--batch' in capsys.readouterr().err
    assert L.main(['make', '--sequence', str(s), '--output_folder', out, '--depth_focal_x', '-3']) == 1
    assert 'positive' in capsys.readouterr().err
    assert L.main(['make', '--sequence', str(tmp_path / 'nowhere'), '--output_folder', out]) == 1
    assert 'nowhere' in capsys.readouterr().err
    os.remove(str(s / 'frame-000001.depth.png'))
    assert L.main(['make', '--sequence', str(s), '--output_folder', out]) == 1
    assert 'frame-000001.depth.png is missing' in capsys.readouterr().err
    assert L.main([]) == 1
    assert not os.path.exists(out)                # nothing was written by a refused call
    r = _run('kfnet_amd.labels', 'make', '--output_folder', out)
    assert r.returncode == 1 and '--sequence' in r.stderr


def test_train_depth_argument_errors(tmp_path, capsys):
    from kfnet_amd.SCoordNet import train as T
    base = ['--scene', 'fire', '--model_folder', str(tmp_path / 'm')]
    assert T.main(base + ['--depth', '--synthetic', '4']) == 1
    assert '--synthetic' in capsys.readouterr().err
    empty = tmp_path / 'in'
    os.makedirs(str(empty))
    assert T.main(base + ['--depth', '--input_folder', str(empty)]) == 1
    assert 'image_list.txt' in capsys.readouterr().err
    # lists without transform.txt
    s = tmp_path / 's'
    _touch_sequence(s, range(2))
    for name, col in zip(L.LISTS, zip(*read_sequence(str(s)))):
        with open(str(empty / name), 'w') as f:
            f.write(''.join(p + '\n' for p in col))
    assert T.main(base + ['--depth', '--input_folder', str(empty)]) == 1
    assert 'transform.txt' in capsys.readouterr().err
    np.savetxt(str(empty / 'transform.txt'), np.eye(4))
    os.remove(str(s / 'frame-000001.depth.png'))
    assert T.main(base + ['--depth', '--input_folder', str(empty)]) == 1
    assert 'frame-000001.depth.png is missing' in capsys.readouterr().err
    assert T.main(base + ['--depth', '--input_folder', str(empty), '--focal_x', '0']) == 1
    assert 'positive' in capsys.readouterr().err
    a = T.build_parser().parse_args(base)
    assert a.depth is False and a.focal_x == 525.0 and a.depth_focal_x is None


# -- 8. the new exports' argument checks: KFN_ERR_ARG with nothing launched, so no device is needed -------------------------
def _labels_call(d, depth=0x1000, poses=0x1000, out=0x1000):
    lib = _lib.load()
    return lib.kfn_depth_labels(C.byref(d), depth, poses, out, None), lib.kfn_last_error().decode()


def test_depth_labels_argument_checks():
    ok = dict(B=1, H=16, W=24, stride=8)
    for change, word in ((dict(stride=2), 'stride'), (dict(stride=0), 'stride'), (dict(H=20), 'multiples of 8'),
                         (dict(W=30), 'multiples of 8'), (dict(H=0), 'multiples of 8'), (dict(B=0), 'multiples of 8'),
                         (dict(ld_out=3), 'ld_out')):
        rc, msg = _labels_call(CAM.descriptor(**dict(ok, **change)))
        assert rc == -1 and word in msg, (change, msg)
    d = CAM.descriptor(**ok)
    d.struct_size -= 4
    rc, msg = _labels_call(d)
    assert rc == -1 and 'struct_size' in msg
    for null in ('depth', 'poses', 'out'):
        rc, msg = _labels_call(CAM.descriptor(**ok), **{null: None})
        assert rc == -1 and 'null' in msg
    assert _lib.load().kfn_depth_labels(None, 0x1000, 0x1000, 0x1000, None) == -1


def test_label_moments_argument_checks():
    lib = _lib.load()

    def call(d, labels=0x1000, partial=0x1000):
        return lib.kfn_label_moments(C.byref(d), labels, partial, None), lib.kfn_last_error().decode()
    ok = dict(B=1, h=4, w=6, ld=4)
    assert C.sizeof(_lib.LabelMomentsDesc) == 48
    for change, word in ((dict(ld=3), 'ld'), (dict(B=0), 'shape'), (dict(h=0), 'shape'), (dict(w=-1), 'shape')):
        rc, msg = call(_lib.LabelMomentsDesc(**dict(ok, **change)))
        assert rc == -1 and word in msg, (change, msg)
    d = _lib.LabelMomentsDesc(**ok)
    d.struct_size += 8
    rc, msg = call(d)
    assert rc == -1 and 'struct_size' in msg
    for null in ('labels', 'partial'):
        rc, msg = call(_lib.LabelMomentsDesc(**ok), **{null: None})
        assert rc == -1 and 'null' in msg
    assert lib.kfn_label_moments(None, 0x1000, 0x1000, None) == -1


# -- 9. the ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_number_stays_and_the_new_symbols_are_exported():
    lib = _lib.load()
    assert lib.kfn_abi_version() == 13 and _lib.ABI_VERSION == 13
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ('kfn_decode_png_gray16', 'kfn_depth_labels', 'kfn_label_moments'):
        assert name in _lib.SYMBOLS and getattr(raw, name) is not None
    hdr = open(os.path.join(ROOT, 'include', 'kfnet_hip.h')).read()
    assert '#define KFN_ABI_VERSION 13' in hdr
    for name in ('kfn_depth_labels_desc', 'kfn_label_moments_desc'):
        assert 'typedef struct %s {' % name in hdr
    from kfnet_amd import build
    assert build.EXTRA['kfn_labels.hip'] == ['-ffp-contract=off']
