"""aefft_frames_register restated in numpy, in double precision (include/aefft.h "aefft_frames_register_ref, aefft_frames_register"): the window,
the kept bins and their count K, the normalised cross-power, the surface, the peak with its tie rule, the 5 x 5 centroid and the wrap to signed
shifts -- and the texture construction the accuracy tests share.  A plain module: pytest collects nothing from it and the product never imports it."""
import numpy as np

WINDOW = {"hann": 0, "nowindow": 1}          # AEFFT_REGISTER_HANN, AEFFT_REGISTER_NOWINDOW
Q = 1 << 24
CHUNK = 4096                                 # cells of a stage-one workgroup of the peak


def spec_floats(Nx, Ny):
    return 2 * Nx * (Ny // 2 + 1) if size_ok(Nx) and size_ok(Ny) else 0


def size_ok(n):
    """a power of two in 8..2048 or an even size in 10..2048 with no prime factor above 5"""
    if n < 8 or n > 2048 or n % 2:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def workspace(Nx, Ny, B):
    if not (size_ok(Nx) and size_ok(Ny)) or B < 1 or B * Nx * Ny >= 1 << 29:
        return 0
    r16 = lambda v: (v + 15) & ~15
    return r16(4 * B * Nx * Ny) + r16(8 * B * Nx * (Ny // 2 + 1)) + r16(8 * B * -(-Nx * Ny // CHUNK))


def window(N, kind):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N) if kind == "hann" else np.ones(N)


def kept(Nx, Ny, kind, cutoff):
    """the kept bins of the FULL Nx x Ny spectrum as a boolean [Nx][Ny]; cutoff is the float the call receives"""
    c = float(np.float32(cutoff))
    u = np.minimum(np.arange(Nx), Nx - np.arange(Nx))[:, None]
    v = np.minimum(np.arange(Ny), Ny - np.arange(Ny))[None, :]
    low = 1 if kind == "hann" else 0
    return (2 * u <= c * Nx) & (2 * v <= c * Ny) & ~((u <= low) & (v <= low))


def prepare(frames, kind):
    """[B][D][Nx][Ny] -> the windowed channel sum [B][Nx][Ny]"""
    f = np.asarray(frames, np.float64)
    Nx, Ny = f.shape[-2:]
    return f.sum(1) * window(Nx, kind)[:, None] * window(Ny, kind)[None, :]


def spectrum(frames, kind):
    return np.fft.rfft2(prepare(frames, kind))


def surface(frames, ref, kind="hann", cutoff=0.5):
    """frames [B][D][Nx][Ny], ref [1 or B][D][Nx][Ny] -> s [B][Nx][Ny]"""
    Nx, Ny = np.shape(frames)[-2:]
    G, Gr = spectrum(frames, kind), spectrum(ref, kind)
    R = G * np.conj(Gr)
    m = np.abs(R)
    keep = kept(Nx, Ny, kind, cutoff)
    K = int(keep.sum())
    assert K > 0
    Qs = np.where(keep[:, :Ny // 2 + 1] & (m > 0), R / np.where(m > 0, m, 1.0), 0.0)
    return np.fft.irfft2(Qs, s=(Nx, Ny)) * (Nx * Ny) / K


def peak(s):
    """one surface [Nx][Ny] -> (dx, dy, response, cell)"""
    Nx, Ny = s.shape
    cell = int(np.argmax(np.where(np.isnan(s), -np.inf, s)))                      # (numpy's argmax: the first of equals)
    pi, pj = divmod(cell, Ny)
    sw = si = sj = 0.0
    for di in range(-2, 3):
        for dj in range(-2, 3):
            w = max(float(s[(pi + di) % Nx, (pj + dj) % Ny]), 0.0)
            sw += w
            si += w * di
            sj += w * dj
    dx = pi + (si / sw if sw > 0 else 0.0)
    dy = pj + (sj / sw if sw > 0 else 0.0)
    if dx >= Nx // 2:
        dx -= Nx
    if dy >= Ny // 2:
        dy -= Ny
    return dx, dy, float(s[pi, pj]), cell


def register(frames, ref, kind="hann", cutoff=0.5):
    """-> ([B] of (dx, dy, response, cell), the surfaces)"""
    s = surface(frames, ref, kind, cutoff)
    return [peak(x) for x in s], s


def peak_gap(s):
    """the largest surface value minus the second largest"""
    top = np.sort(np.ravel(s))[-2:]
    return float(top[1] - top[0])


def affine(dx, dy, response, min_response, scale):
    """the six Q24 coefficients from the DEVICE's float dx, dy and response"""
    if not float(response) >= float(np.float32(min_response)):
        return [Q, 0, 0, 0, Q, 0]
    return [Q, 0, int(np.rint(np.float64(np.float32(dx)) * np.float64(scale[0]) * 16777216.0)), 0, Q,
            int(np.rint(np.float64(np.float32(dy)) * np.float64(scale[1]) * 16777216.0))]


# ------------------------------------------------------------------------------------------
# the texture construction: Gaussian-low-passed noise on a 2 x canvas, cropped at an offset, quantised to 8 bits -- the shift is not circular
# ------------------------------------------------------------------------------------------
def canvas(Nx, Ny, seed, D=1, sigma=0.08):
    """[D][2 Nx][2 Ny] doubles around 128: white noise through exp(-f^2 / (2 sigma^2)), f in cycles per pixel"""
    rng = np.random.default_rng(seed)
    fx, fy = np.fft.fftfreq(2 * Nx)[:, None], np.fft.fftfreq(2 * Ny)[None, :]
    H = np.exp(-(fx * fx + fy * fy) / (2.0 * sigma * sigma))
    out = []
    for _ in range(D):
        t = np.fft.ifft2(np.fft.fft2(rng.standard_normal((2 * Nx, 2 * Ny))) * H).real
        out.append(128.0 + 48.0 * t / t.std())
    return np.stack(out)


def crop(c, Nx, Ny, sx=0.0, sy=0.0):
    """the Nx x Ny window of the canvas whose content is the centred window's moved by (+sx, +sy): img(x) = ref(x - s).  A fractional shift is a phase
    ramp on the (periodic) canvas.  Quantised to 8 bits."""
    D, Cx, Cy = c.shape
    fx, fy = np.fft.fftfreq(Cx)[:, None], np.fft.fftfreq(Cy)[None, :]
    moved = np.fft.ifft2(np.fft.fft2(c) * np.exp(-2j * np.pi * (fx * sx + fy * sy))).real
    x0, y0 = Cx // 4, Cy // 4
    return np.clip(np.rint(moved[:, x0:x0 + Nx, y0:y0 + Ny]), 0, 255).astype(np.uint8)


def texture_pair(Nx, Ny, seed, shift, D=1):
    """(ref, img) uint8 [D][Nx][Ny] with img the reference moved by `shift`"""
    c = canvas(Nx, Ny, seed, D)
    return crop(c, Nx, Ny), crop(c, Nx, Ny, *shift)
