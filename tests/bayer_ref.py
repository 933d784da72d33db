"""aefft_raw_to_image restated in numpy (int64) from the text of include/aefft.h alone: unpacking of the three containers, step 1 (linearise), step 2
(reflected borders), step 3 (BILINEAR and MHC as whole-image shifted sums), step 4 (colour matrix), step 5 (byte or table), step 6 (MONO).  A plain
module -- pytest collects nothing from it -- that shares nothing with the kernel or the host check."""
import math

import numpy as np

PATTERNS = ("rggb", "grbg", "gbrg", "bggr", "mono")
CONTAINERS = ("u8", "u16", "packed")
METHODS = ("bilinear", "mhc")
FULL = 255 << 16
# the colour (0 R, 1 G, 2 B) of pixels (0,0), (1,0) of row 0 and (0,1), (1,1) of row 1: GenICam's naming
COLOURS = {"rggb": ((0, 1), (1, 2)), "grbg": ((1, 0), (2, 1)), "gbrg": ((1, 2), (0, 1)), "bggr": ((2, 1), (1, 0))}
# the MHC filters in sixteenths as 5 x 5 tables [dy + 2][dx + 2], written out from the header's sums
MHC_G = [[0, 0, -2, 0, 0], [0, 0, 4, 0, 0], [-2, 4, 8, 4, -2], [0, 0, 4, 0, 0], [0, 0, -2, 0, 0]]            # G at an R/B site
MHC_ROW = [[0, 0, 1, 0, 0], [0, -2, 0, -2, 0], [-2, 8, 10, 8, -2], [0, -2, 0, -2, 0], [0, 0, 1, 0, 0]]       # R at a G site, R in the same row
MHC_COL = [list(r) for r in zip(*MHC_ROW)]                                                                    # ... in the same column: the transpose
MHC_DIAG = [[0, 0, -3, 0, 0], [0, 4, 0, 4, 0], [-3, 0, 12, 0, -3], [0, 4, 0, 4, 0], [0, 0, -3, 0, 0]]        # R at a B site
BIL_G = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
BIL_ROW = [[0, 0, 0], [1, 0, 1], [0, 0, 0]]
BIL_COL = [[0, 1, 0], [0, 0, 0], [0, 1, 0]]
BIL_DIAG = [[1, 0, 1], [0, 0, 0], [1, 0, 1]]


def row_bytes(container, bits, W):
    return {"u8": W, "u16": 2 * W, "packed": (W * bits + 7) // 8}[container]


def pack(samples, bits):
    """samples [..][W] -> the bytes [..][ceil(W bits / 8)] of GenICam's 10p / 12p: sample x in bits [x bits, (x + 1) bits) of a little-endian bit stream"""
    s = np.asarray(samples, dtype=np.int64)
    W = s.shape[-1]
    out = np.zeros(s.shape[:-1] + ((W * bits + 7) // 8,), dtype=np.int64)
    for x in range(W):
        for k in range(bits):
            pos = x * bits + k
            out[..., pos // 8] |= ((s[..., x] >> k) & 1) << (pos % 8)
    return out.astype(np.uint8)


def unpack(rows, bits, W):
    """the inverse of pack, over the first ceil(W bits / 8) bytes of each row"""
    r = np.asarray(rows, dtype=np.int64)
    out = np.zeros(r.shape[:-1] + (W,), dtype=np.int64)
    for x in range(W):
        for k in range(bits):
            pos = x * bits + k
            out[..., x] |= ((r[..., pos // 8] >> (pos % 8)) & 1) << k
    return out


def multiplier(gain, black, white):
    """m_c: once on the host, in double (gain as the float the descriptor holds)"""
    return int(math.floor(float(np.float32(gain)) * 255.0 * 65536.0 / float(white - black) + 0.5))


def colour_map(pattern, W, H):
    """[H][W] of 0 R, 1 G, 2 B"""
    c = np.array(COLOURS[pattern], dtype=np.int64)
    return c[np.arange(H)[:, None] % 2, np.arange(W)[None, :] % 2]


def linearise(samples, pattern, black, white, gains):
    """step 1 over samples [..][H][W] (int64): u in Q16"""
    s = np.maximum(np.asarray(samples, dtype=np.int64) - black, 0)
    H, W = s.shape[-2:]
    if pattern == "mono":
        m = np.int64(multiplier(gains[0], black, white))
    else:
        m = np.array([multiplier(g, black, white) for g in gains], dtype=np.int64)[colour_map(pattern, W, H)]
    return np.minimum(s * m, FULL)


def reflect(i, n):
    """step 2, for any index with a reach below n"""
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _filter(u, table):
    """the sum of table[dy + r][dx + r] * u(y + dy, x + dx) at every pixel, the borders reflected"""
    H, W = u.shape[-2:]
    r = len(table) // 2
    acc = np.zeros_like(u)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            k = table[dy + r][dx + r]
            if k:
                acc += k * u[..., reflect(np.arange(H) + dy, H)[:, None], reflect(np.arange(W) + dx, W)[None, :]]
    return acc


def demosaic(u, pattern, method):
    """step 3: u [..][H][W] -> v [..][H][W][3] as (R, G, B)"""
    H, W = u.shape[-2:]
    col = colour_map(pattern, W, H)
    if method == "mhc":
        f = lambda t: np.clip((_filter(u, t) + 8) >> 4, 0, FULL)
        g, row, colm, diag = f(MHC_G), f(MHC_ROW), f(MHC_COL), f(MHC_DIAG)
    else:
        g, diag = (_filter(u, BIL_G) + 2) >> 2, (_filter(u, BIL_DIAG) + 2) >> 2
        row, colm = (_filter(u, BIL_ROW) + 1) >> 1, (_filter(u, BIL_COL) + 1) >> 1
    out = np.zeros(u.shape + (3,), dtype=np.int64)
    # the colour of the non-green sites of every pixel's row (a row of the mosaic is R G R G .. or G B G B ..)
    row_colour = np.broadcast_to(np.array([[c for c in COLOURS[pattern][j] if c != 1][0] for j in (0, 1)])[np.arange(H) % 2][:, None], (H, W))
    for c in (0, 2):                                       # "R" swaps with B by symmetry
        at_g_same_row = (col == 1) & (row_colour == c)
        at_g_same_col = (col == 1) & (row_colour == 2 - c)
        out[..., c] = np.where(col == c, u, np.where(col == 2 - c, diag, np.where(at_g_same_row, row, colm)))
        assert (at_g_same_row | at_g_same_col | (col != 1)).all()
    out[..., 1] = np.where(col == 1, u, g)
    return out


def quantise_ccm(ccm):
    if ccm is None:
        return np.eye(3, dtype=np.int64) * 1024
    m = np.asarray(ccm, dtype=np.float32).astype(np.float64).reshape(3, 3)
    return np.floor(m * 1024.0 + 0.5).astype(np.int64)


def to_byte(o, lut):
    """step 5"""
    if lut is None:
        return np.clip((o + (1 << 17)) >> 18, 0, 255).astype(np.uint8)
    return np.asarray(lut, dtype=np.uint8).reshape(-1)[np.clip((o + (1 << 13)) >> 14, 0, 4080)]


def raw_to_image(samples, pattern, black=0, white=255, gains=(1, 1, 1), method="mhc", order="bgr", ccm=None, lut=None):
    """the image [B][H][W][D] (uint8) of the samples [B][H][W] (the values r, whatever the container)"""
    u = linearise(samples, pattern, black, white, gains)
    if pattern == "mono":
        return to_byte(1024 * ((u + 128) >> 8), lut)[..., None]
    q = (demosaic(u, pattern, method) + 128) >> 8
    o = np.einsum("ij,...j->...i", quantise_ccm(ccm), q)
    img = to_byte(o, lut)
    return img[..., ::-1].copy() if order == "bgr" else img


def samples_of(data, container, bits, W):
    """the values r of raw rows as the containers hold them: u8 [..][>= W] bytes, u16 [..][>= W] words (the low `bits` bits), packed [..][bytes]"""
    if container == "u8":
        return np.asarray(data)[..., :W].astype(np.int64)
    if container == "u16":
        return np.asarray(data)[..., :W].astype(np.int64) & ((1 << bits) - 1)
    return unpack(data, bits, W)


def gamma_lut(gamma):
    """aefft.gamma_lut's stated formula, in double"""
    x = np.minimum(np.arange(4096), 4080) / 4080.0
    return np.floor(255.0 * x ** (1.0 / gamma) + 0.5).astype(np.uint8)


def srgb_lut():
    x = np.minimum(np.arange(4096), 4080) / 4080.0
    return np.floor(255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055) + 0.5).astype(np.uint8)
