"""The yardstick of the JPEG round trip (csrc/jpeg.hip): the baseline codec with libjpeg's default "islow" integer DCT, restated
in numpy with int64 throughout.  ``jpeg_roundtrip(img, quality, subsampling)`` is what
``PIL.Image.fromarray(img).save(f, 'JPEG', quality=q, subsampling=0|2)`` followed by ``Image.open(f)`` gives, bit for bit
(tests/test_host_jpeg.py holds it against Pillow itself).  No bitstream is made: entropy coding is lossless.  No product code
is used here."""
import numpy as np

UNIT, LR_REF, HR_REF, HR_UNIT = range(4)

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64).reshape(8, 8)

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def F(x):
    return int(x * 65536 + 0.5)


def DS(x, n):
    return (x + (1 << (n - 1))) >> n


def quant_table(base, quality):
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def fdct_1d(d, first):
    """jfdctint along the last axis of int64 [..., 8]; first: pass 1 (rows) or pass 2 (columns)"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else DS(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else DS(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = DS(z1 + t13 * F_0_765, n)
    o[6] = DS(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = DS(t4 + z1 + z3, n), DS(t5 + z2 + z4, n), DS(t6 + z2 + z3, n), DS(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def idct_1d(c, n):
    """jidctint along the last axis of int64 [..., 8], descaled by n (11: pass 1, columns; 18: pass 2, rows)"""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * F_0_541
    t2, t3 = z1 - c[6] * F_1_847, z1 + c[2] * F_0_765
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    o = [DS(t10 + t3, n), DS(t11 + t2, n), DS(t12 + t1, n), DS(t13 + t0, n),
         DS(t13 - t0, n), DS(t12 - t1, n), DS(t11 - t2, n), DS(t10 - t3, n)]
    return np.stack(o, axis=-1)


def codec_plane(plane, table):
    """int64 [Hp, Wp] (multiples of 8) samples 0..255 -> the decoded samples: FDCT, quantise, dequantise, IDCT per 8x8 block"""
    hp, wp = plane.shape
    b = plane.reshape(hp // 8, 8, wp // 8, 8).transpose(0, 2, 1, 3) - 128          # [by][bx][row][col]
    c = fdct_1d(b, True)                                                            # rows
    c = fdct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                         # columns
    d = table << 3
    k = (np.abs(c) + (d >> 1)) // d
    c = np.where(c < 0, -k, k) * table
    w = idct_1d(c.swapaxes(-1, -2), 11).swapaxes(-1, -2)                            # columns
    o = np.clip(idct_1d(w, 18) + 128, 0, 255)                                       # rows
    return o.transpose(0, 2, 1, 3).reshape(hp, wp)


def pad_edge(plane, hp, wp):
    return np.pad(plane, ((0, hp - plane.shape[0]), (0, wp - plane.shape[1])), mode="edge")


def upsample_fancy(c):
    """[ch, cw] real chroma samples, cw > 2 -> [2 ch, 2 cw]: libjpeg's h2v2 triangle filter"""
    ch, cw = c.shape
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    cs = np.empty((2 * ch, cw), dtype=np.int64)
    cs[0::2], cs[1::2] = 3 * c + above, 3 * c + below
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 2::2] = (3 * cs[:, 1:] + cs[:, :-1] + 8) >> 4
    out[:, 1:-1:2] = (3 * cs[:, :-1] + cs[:, 1:] + 7) >> 4
    out[:, 0] = (4 * cs[:, 0] + 8) >> 4
    out[:, -1] = (4 * cs[:, -1] + 7) >> 4
    return out


def jpeg_roundtrip(img, quality, subsampling):
    """uint8 [H, W, 3] RGB -> uint8 [H, W, 3]; subsampling 0 (4:4:4) or 2 (4:2:0), quality an integer in 1..100"""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and subsampling in (0, 2)
    H, W = img.shape[:2]
    m = 8 if subsampling == 0 else 16
    hp, wp = -(-H // m) * m, -(-W // m) * m
    p = np.pad(img.astype(np.int64), ((0, hp - H), (0, wp - W), (0, 0)), mode="edge")
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (F(.299) * r + F(.587) * g + F(.114) * b + 32768) >> 16
    cb = (-F(.16874) * r - F(.33126) * g + F(.5) * b + (128 << 16) + 32767) >> 16
    cr = (F(.5) * r - F(.41869) * g - F(.08131) * b + (128 << 16) + 32767) >> 16
    tl, tc = quant_table(LUMA, quality), quant_table(CHROMA, quality)
    y = codec_plane(y, tl)
    if subsampling == 0:
        cb, cr = codec_plane(cb, tc), codec_plane(cr, tc)
    else:
        ch, cw = -(-H // 2), -(-W // 2)
        bias = np.tile(np.array([1, 2], dtype=np.int64), wp // 4)

        def down(c):
            d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
            d[ch:] = d[ch - 1]
            return d

        def up(c):
            c = c[:ch, :cw]
            full = upsample_fancy(c) if cw > 2 else np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
            return pad_edge(full, hp, wp)                               # only [:H, :W] is kept below

        cb, cr = up(codec_plane(down(cb), tc)), up(codec_plane(down(cr), tc))
    cb, cr = cb - 128, cr - 128
    out = np.stack([y + ((F(1.402) * cr + 32768) >> 16),
                    y + ((-F(.34414) * cb + 32768 - F(.71414) * cr) >> 16),
                    y + ((F(1.772) * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255)[:H, :W].astype(np.uint8)


def levels_f32(x):
    """fp32 [..., 3, h, w] in PATCH_UNIT scaling -> uint8 [..., h, w, 3]: (int)rintf(min(max(255 * v, 0), 255)), 255 * v in fp32"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    v = np.rint(np.clip(np.float32(255.0) * x, np.float32(0.0), np.float32(255.0))).astype(np.uint8)
    return np.moveaxis(v, -3, -1)


def scale_f32(u8, mode):
    """uint8 [..., h, w, 3] -> fp32 [..., 3, h, w] as dsr_patch_batch_u8 scales it: /255.0f, then the statements of `mode`"""
    f = np.float32
    v = np.moveaxis(u8, -1, -3).astype(f) / f(255)
    if mode == LR_REF:
        v = v / f(255)
    elif mode == HR_REF:
        v = v / f(255)
        v = v * f(2)
        v = v - f(1)
    elif mode == HR_UNIT:
        v = v * f(2)
        v = v - f(1)
    assert v.dtype == f
    return np.ascontiguousarray(v)
