"""The numpy int64 restatement of aefft_image_to_yuv (include/aefft.h): luma per pixel, chroma the rounded box average over a sample's LIVE pixels,
laid out as planes.  The tests' oracle; the product never imports it."""
import numpy as np

# matrix -> (yoff, ky, (r, g, b) of Y, of U, of V): include/aefft.h's table
TABLE = {
    "bt601": (16, 900542, (269262, 528618, 102662), (-155423, -305128, 460551), (460551, -385654, -74897)),
    "bt709": (16, 900542, (191455, 644068, 65019), (-105533, -355018, 460551), (460551, -418321, -42230)),
    "jpeg": (0, 1048576, (313524, 615514, 119538), (-176932, -347356, 524288), (524288, -439026, -85262)),
}
FORMATS, MATRICES, ORDERS = ("nv12", "i420", "yuyv"), ("bt601", "bt709", "jpeg"), ("bgr", "rgb", "gray")


def _constants(matrix):
    kr, kb = (0.2126, 0.0722) if matrix == "bt709" else (0.299, 0.114)
    sy, sc, yoff = (1.0, 1.0, 0) if matrix == "jpeg" else (219.0 / 255.0, 224.0 / 255.0, 16)
    return kr, kb, sy, sc, yoff


def real_coefficients(matrix):
    """(yoff, (r, g, b) of Y, of U, of V) as real numbers: what the table quantises"""
    kr, kb, sy, sc, yoff = _constants(matrix)
    kg = 1.0 - kr - kb
    return (yoff, (kr * sy, kg * sy, kb * sy), (-kr * sc / (2 * (1 - kb)), -kg * sc / (2 * (1 - kb)), sc / 2),
            (sc / 2, -kg * sc / (2 * (1 - kr)), -kb * sc / (2 * (1 - kr))))


def derive(matrix):
    """the table's entry from the standards' constants, in double; the G entries are the remainders: the Y row sums to ky, the U and V rows to 0"""
    kr, kb, sy, sc, yoff = _constants(matrix)
    q = lambda k: int(round(k * 2.0 ** 20))
    ky, yr, yb = q(sy), q(kr * sy), q(kb * sy)
    ub = vr = q(sc / 2)
    ur, vb = q(-kr * sc / (2 * (1 - kb))), q(-kb * sc / (2 * (1 - kr)))
    return yoff, ky, (yr, ky - yr - yb, yb), (ur, -(ur + ub), ub), (vr, -(vr + vb), vb)


def _rgb(img, order):
    """uint8 [...][D] -> int64 R, G, B (gray: the one channel three times)"""
    p = img.astype(np.int64)
    if order == "gray":
        assert p.shape[-1] == 1
        return p[..., 0], p[..., 0], p[..., 0]
    assert p.shape[-1] == 3
    return (p[..., 2], p[..., 1], p[..., 0]) if order == "bgr" else (p[..., 0], p[..., 1], p[..., 2])


def luma(img, matrix, order):
    yoff, ky, (yr, yg, yb), _, _ = TABLE[matrix]
    R, G, B = _rgb(img, order)
    t = ky * R if order == "gray" else yr * R + yg * G + yb * B
    return (yoff + ((t + 2 ** 19) >> 20)).astype(np.uint8)


def pixel_yuv(R, G, B, matrix):
    """integer arrays of one shape -> Y, U, V (int64) of pixels whose chroma sample is their own (n = 1)"""
    yoff, _, ky, ku, kv = TABLE[matrix]
    R, G, B = (np.asarray(c).astype(np.int64) for c in (R, G, B))
    f = lambda k: (k[0] * R + k[1] * G + k[2] * B + 2 ** 19) >> 20
    return yoff + f(ky), np.clip(128 + f(ku), 0, 255), np.clip(128 + f(kv), 0, 255)


def _block_sums(c, fy, fx):
    """int64 [B][H][W] -> (the sums over blocks of fy x fx cut to the image, the counts n of live pixels): [B][ceil(H / fy)][ceil(W / fx)]"""
    B, H, W = c.shape
    Hp, Wp = -(-H // fy) * fy, -(-W // fx) * fx
    z = np.zeros((B, Hp, Wp), dtype=np.int64)
    z[:, :H, :W] = c
    one = np.zeros((1, Hp, Wp), dtype=np.int64)
    one[:, :H, :W] = 1
    blk = lambda a: a.reshape(a.shape[0], Hp // fy, fy, Wp // fx, fx).sum(axis=(2, 4))
    return blk(z), blk(one)[0]


def chroma(img, matrix, order, fy):
    """U, V [B][ceil(H / fy)][ceil(W / 2)]: fy = 2 for nv12 and i420, 1 for yuyv"""
    _, _, _, ku, kv = TABLE[matrix]
    R, G, B = _rgb(img, order)
    if order == "gray":
        n = _block_sums(R, fy, 2)[0]
        return np.full(n.shape, 128, np.uint8), np.full(n.shape, 128, np.uint8)
    (SR, n), (SG, _), (SB, _) = (_block_sums(c, fy, 2) for c in (R, G, B))
    assert set(np.unique(n)) <= {1, 2, 4}
    lg = np.log2(n).astype(np.int64)[None]
    out = []
    for kr, kg, kb in (ku, kv):
        t = kr * SR + kg * SG + kb * SB
        assert np.abs(t).max() < 2 ** 30
        out.append(np.clip(128 + ((t + (n[None] << 19)) >> (20 + lg)), 0, 255).astype(np.uint8))      # (>> on int64: arithmetic, the floor)
    return out


def image_to_yuv(img, fmt, matrix="bt601", order="bgr"):
    """img uint8 [B][H][W][D] -> the planes as Context.image_to_yuv returns them (numpy, batched)"""
    Y = luma(img, matrix, order)
    U, V = chroma(img, matrix, order, 1 if fmt == "yuyv" else 2)
    if fmt == "nv12":
        return (Y, np.ascontiguousarray(np.stack([U, V], axis=-1)))
    if fmt == "i420":
        return (Y, U, V)
    B, H, W = Y.shape
    assert W % 2 == 0
    return (np.ascontiguousarray(np.stack([Y[:, :, 0::2], U, Y[:, :, 1::2], V], axis=-1)),)
