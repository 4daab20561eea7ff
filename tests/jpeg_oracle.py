"""A baseline JPEG round trip (encode at a quality, decode) restated in numpy integers, for the tests: the checker of
sr_gan_fd_amd/csrc/jpeg.hip on machines without an image library.  It follows libjpeg's default pipeline as libjpeg-turbo and cv2's
``imencode`` / ``imdecode`` run it -- 4:2:0, the slow-but-accurate integer DCT, fancy upsampling -- and equals Pillow's
``save(quality=q)`` / ``open`` byte for byte (tests/test_bsrgan_degradation_host.py checks that where Pillow imports).  Entropy coding is
lossless and does not appear.

  roundtrip_u8(rgb, quality)   (H, W, 3) uint8 -> (H, W, 3) uint8
  roundtrip(image, quality)    (3, H, W) float, any range -> float32: uint8(round(clip(x, 0, 1) * 255)), the round trip, float32(u8) / 255

The steps: RGB -> YCbCr from 16-bit fixed-point products; columns replicated at the right edge to a multiple of 16; chroma averaged
2 x 2 with the bias 1, 2, 1, 2 ... along a row (an odd height's last row doubled first); luma rows replicated to a multiple of 16 and
the averaged chroma rows to a multiple of 8 -- so the last chroma row of an even height is a real average of two rows, repeated; per
8 x 8 block the forward DCT (13-bit constants, two passes), quantisation (|c| + 4 q) / (8 q) with the sign put back, the product with q,
the inverse DCT and the + 128 clamp; chroma cropped to ceil(h / 2) x ceil(w / 2) and enlarged with the 3:1 triangle filter in both
directions (biases 8 and 7, edge rows and columns repeated; a chroma plane of one or two columns is repeated 2 x 2 instead, as the
library does); YCbCr -> RGB.  Everything fits int32; int64 is used for convenience."""
import numpy as np

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA = np.full((8, 8), 99, dtype=np.int64)
CHROMA[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def fix(x):
    return int(x * 65536 + 0.5)


def quant_table(base, quality):
    quality = min(max(int(quality), 1), 100)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * s + 50) // 100, 1, 255)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, first):
    """one pass of the forward DCT along the last axis of an int64 array (..., 8)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = descale(z1 + t13 * F_0_765, n)
    o[6] = descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def idct_pass(d, first):
    """one pass of the inverse DCT along the last axis"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., i] for i in range(8))
    z1 = (i2 + i6) * F_0_541
    t2, t3 = z1 - i6 * F_1_847, z1 + i2 * F_0_765
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return np.stack([descale(t10 + t3, n), descale(t11 + t2, n), descale(t12 + t1, n), descale(t13 + t0, n),
                     descale(t13 - t0, n), descale(t12 - t1, n), descale(t11 - t2, n), descale(t10 - t3, n)], axis=-1)


def code_plane(p, q):
    """(H8, W8) int64 samples, both multiples of 8 -> the decoded samples: DCT, quantise, dequantise, inverse DCT per block"""
    h, w = p.shape
    b = p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128            # (by, bx, row, col)
    c = fdct_pass(b, True)                                                     # rows
    c = fdct_pass(c.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)        # columns
    a = (np.abs(c) + 4 * q) // (8 * q)
    c = np.where(c < 0, -a, a) * q
    c = idct_pass(c.transpose(0, 1, 3, 2), True).transpose(0, 1, 3, 2)         # columns
    c = idct_pass(c, False)                                                    # rows
    return np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def upsample_fancy(c):
    """(h2, w2) chroma -> (2 h2, 2 w2): rows 3:1 with the neighbouring row (edge rows repeated), then columns with biases 8 / 7"""
    h2, w2 = c.shape
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    rows = np.empty((2 * h2, w2), dtype=np.int64)
    rows[0::2], rows[1::2] = 3 * c + up, 3 * c + down
    if w2 <= 2:
        raise AssertionError("the caller repeats narrow planes")
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((2 * h2, 2 * w2), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return out


def roundtrip_u8(rgb, quality):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w = rgb.shape[:2]
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + (128 << 16) + half - 1) >> 16
    cr = (fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    # the library replicates columns before it downsamples, and rows after (an odd height's last row is first doubled)
    y = np.pad(y, ((0, -h % 16), (0, -w % 16)), mode="edge")
    cb, cr = (np.pad(p, ((0, h % 2), (0, -w % 16)), mode="edge") for p in (cb, cr))
    bias = np.tile(np.array([1, 2], dtype=np.int64), y.shape[1] // 4)[None, :]
    cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2 for p in (cb, cr))
    cb, cr = (np.pad(p, ((0, -p.shape[0] % 8), (0, 0)), mode="edge") for p in (cb, cr))
    y = code_plane(y, quant_table(LUMA, quality))[:h, :w]
    qc = quant_table(CHROMA, quality)
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    cb, cr = (code_plane(p, qc)[:h2, :w2] for p in (cb, cr))
    if w2 > 2:
        cb, cr = (upsample_fancy(p)[:h, :w] for p in (cb, cr))
    else:
        cb, cr = (np.repeat(np.repeat(p, 2, 0), 2, 1)[:h, :w] for p in (cb, cr))
    cb, cr = cb - 128, cr - 128
    out = np.stack([y + ((fix(1.40200) * cr + half) >> 16),
                    y + ((-fix(0.34414) * cb + half - fix(0.71414) * cr) >> 16),
                    y + ((fix(1.77200) * cb + half) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def quantise(image):
    """(3, H, W) float -> (H, W, 3) uint8, as the reference's _add_jpeg_compression does: uint8(round(clip(x, 0, 1) * 255)) in float32"""
    x = np.asarray(image, dtype=np.float32)
    return np.uint8(np.rint(np.clip(x, 0, 1) * np.float32(255.))).transpose(1, 2, 0)


def roundtrip(image, quality):
    if quality == 0:
        return np.asarray(image, dtype=np.float32).copy()
    return (roundtrip_u8(quantise(image), quality).astype(np.float32) / np.float32(255.)).transpose(2, 0, 1)
