"""The numpy int64 restatement of aefft_yuv_to_image (include/aefft.h): gather the chroma (nearest), apply the formula, clamp.  The tests' oracle;
the product never imports it."""
import numpy as np

# matrix -> (yoff, ky, rows (a, b) of R, G, B): include/aefft.h's table
TABLE = {
    "bt601": (16, 1220945, ((0, 1673555), (-410793, -852458), (2115221, 0))),
    "bt709": (16, 1220945, ((0, 1879825), (-223607, -558796), (2215014, 0))),
    "jpeg": (0, 1048576, ((0, 1470104), (-360853, -748826), (1858077, 0))),
}
FORMATS, MATRICES, ORDERS = ("nv12", "i420", "yuyv"), ("bt601", "bt709", "jpeg"), ("bgr", "rgb", "gray")


def derive(matrix):
    """the table's entry from the standards' constants, in double: (yoff, ky, ((a, b) of R, G, B))"""
    kr, kb = (0.2126, 0.0722) if matrix == "bt709" else (0.299, 0.114)
    kg = 1.0 - kr - kb
    sy, sc, yoff = (1.0, 1.0, 0) if matrix == "jpeg" else (255.0 / 219.0, 255.0 / 224.0, 16)
    q = lambda k: int(round(k * 2.0 ** 20))
    return yoff, q(sy), ((0, q(2 * (1 - kr) * sc)), (q(-2 * (1 - kb) * (kb / kg) * sc), q(-2 * (1 - kr) * (kr / kg) * sc)), (q(2 * (1 - kb) * sc), 0))


def real_coefficients(matrix):
    """(yoff, s_y, ((a, b) of R, G, B)) as real numbers: what the table quantises"""
    kr, kb = (0.2126, 0.0722) if matrix == "bt709" else (0.299, 0.114)
    kg = 1.0 - kr - kb
    sy, sc, yoff = (1.0, 1.0, 0) if matrix == "jpeg" else (255.0 / 219.0, 255.0 / 224.0, 16)
    return yoff, sy, ((0.0, 2 * (1 - kr) * sc), (-2 * (1 - kb) * (kb / kg) * sc, -2 * (1 - kr) * (kr / kg) * sc), (2 * (1 - kb) * sc, 0.0))


def convert(Y, U, V, matrix, order):
    """Y, U, V integer arrays of one shape (the chroma already gathered) -> uint8 [..., D]"""
    yoff, ky, rows = TABLE[matrix]
    c, u, v = Y.astype(np.int64) - yoff, U.astype(np.int64) - 128, V.astype(np.int64) - 128
    if order == "gray":
        chans = [ky * c]
    else:
        rgb = [ky * c + a * u + b * v for a, b in rows]
        chans = rgb[::-1] if order == "bgr" else rgb
    out = np.stack(chans, axis=-1)
    assert np.abs(out).max() < 2 ** 30
    return np.clip((out + 2 ** 19) >> 20, 0, 255).astype(np.uint8)       # (>> on int64: arithmetic, the floor)


def gather(planes, fmt, gray=False):
    """planes as Context.yuv_to_image takes them (numpy, batched) -> Y, U, V, each [B][H][W]; with gray the chroma is the neutral 128"""
    if fmt == "yuyv":
        q = planes[0]                                                    # [B][H][W/2][4] = Y0 U Y1 V
        Y = q[..., 0::2].reshape(q.shape[0], q.shape[1], -1)
        U, V = np.repeat(q[..., 1], 2, axis=2), np.repeat(q[..., 3], 2, axis=2)
        return Y, U, V
    Y = planes[0]
    B, H, W = Y.shape
    if gray:
        return Y, np.full_like(Y, 128), np.full_like(Y, 128)
    cu, cv = (planes[1][..., 0], planes[1][..., 1]) if fmt == "nv12" else (planes[1], planes[2])
    yy, xx = np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1
    return Y, cu[:, yy, xx], cv[:, yy, xx]


def yuv_to_image(planes, fmt, matrix="bt601", order="bgr"):
    """uint8 [B][H][W][D]"""
    return convert(*gather(planes, fmt, order == "gray"), matrix, order)


def random_planes(rng, fmt, B, W, H):
    Wc, Hc = (W + 1) // 2, (H + 1) // 2
    r = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    if fmt == "nv12":
        return (r(B, H, W), r(B, Hc, Wc, 2))
    if fmt == "i420":
        return (r(B, H, W), r(B, Hc, Wc), r(B, Hc, Wc))
    assert W % 2 == 0
    return (r(B, H, W // 2, 4),)
