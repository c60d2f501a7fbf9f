"""The procedural shader nodes restated in numpy float32 / uint32, independent of the library's text: the lookup3 hashes,
fade, grad1 / grad2, the lerp order of nd_lerp, the cell rule of tex_floor_to_int, and the math node with its broadcast bits and w rule.
Every operation below is one float32 operation of the definition, in the definition's order: no contraction, no float64 intermediate.
POW alone is not restated: `math_node` takes the function from its caller (pow_f is pinned by the math probes; the node is the subject here).
Shared by tests/test_procedural.py and tests/test_gpu_procedural.py; not a test module."""
import numpy as np

F = np.float32
U = np.uint32

MATH_NAMES = ("add", "sub", "mul", "div", "pow", "min", "max")  # akr_math_op 0..6


# ---------------------------------------------------------------------------------------------- hashes (Blender's lookup3 final)
def _u(x):
    return np.asarray(x).astype(U)


def _rot(x, k):
    return (x << U(k)) | (x >> U(32 - k))


def _final(a, b, c):
    with np.errstate(over="ignore"):
        c = c ^ b; c = c - _rot(b, 14)  # noqa: E702
        a = a ^ c; a = a - _rot(c, 11)  # noqa: E702
        b = b ^ a; b = b - _rot(a, 25)  # noqa: E702
        c = c ^ b; c = c - _rot(b, 16)  # noqa: E702
        a = a ^ c; a = a - _rot(c, 4)  # noqa: E702
        b = b ^ a; b = b - _rot(a, 14)  # noqa: E702
        c = c ^ b; c = c - _rot(b, 24)  # noqa: E702
    return c


def hash_uint(kx):
    kx = _u(kx)
    init = np.full(kx.shape, (0xDEADBEEF + (1 << 2) + 13) & 0xFFFFFFFF, dtype=U)
    with np.errstate(over="ignore"):
        return _final(init + kx, init, init)


def hash_uint2(kx, ky):
    """The y key goes into a, the x key into b."""
    kx, ky = _u(kx), _u(ky)
    init = np.full(kx.shape, (0xDEADBEEF + (2 << 2) + 13) & 0xFFFFFFFF, dtype=U)
    with np.errstate(over="ignore"):
        return _final(init + ky, init + kx, init)


# ---------------------------------------------------------------------------------------------- Perlin
def floor_to_int(x):
    """tex_floor_to_int: NaN and everything below -1e9 become -1e9, everything above 1e9 becomes 1e9; -> (cell as uint32, its float)."""
    x = np.asarray(x, dtype=F)
    lo, hi = F(-1.0e9), F(1.0e9)
    with np.errstate(invalid="ignore"):
        c = np.where(x > lo, x, lo)
        c = np.where(c > hi, hi, c)
    fl = np.floor(c).astype(F)
    return fl.astype(np.int32).view(U), fl


def fade(t):
    return t * t * t * (t * (t * F(6.0) - F(15.0)) + F(10.0))


def grad1(h, x):
    h = h & U(15)
    g = F(1.0) + (h & U(7)).astype(F)
    return np.where((h & U(8)) != 0, -g, g) * x


def grad2(h, x, y):
    h = h & U(7)
    u = np.where(h < 4, x, y)
    v = F(2.0) * np.where(h < 4, y, x)
    return np.where((h & U(1)) != 0, -u, u) + np.where((h & U(2)) != 0, -v, v)


def lerp(a, b, t):
    return a + (b - a) * t


def perlin_1d(x):
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        ix, fl = floor_to_int(x)
        fx = x - fl
        u = fade(fx)
        return lerp(grad1(hash_uint(ix), fx), grad1(hash_uint(ix + U(1)), fx - F(1.0)), u).astype(F)


def perlin_2d(x, y):
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    with np.errstate(all="ignore"):
        ix, flx = floor_to_int(x)
        iy, fly = floor_to_int(y)
        fx, fy = x - flx, y - fly
        u, v = fade(fx), fade(fy)
        c = [grad2(hash_uint2(ix + U(i & 1), iy + U(i >> 1)), fx - F(i & 1), fy - F(i >> 1)) for i in range(4)]  # corner i at (i & 1, i >> 1)
        return lerp(lerp(c[0], c[1], u), lerp(c[2], c[3], u), v).astype(F)  # x first, then y


def noise_node(st, scale, dim):
    """st (n, 2), scale (n,) or a scalar -> (n, 4): (n, 0, 0, 0)."""
    st = np.asarray(st, dtype=F)
    scale = np.broadcast_to(np.asarray(scale, dtype=F), st.shape[:1])
    with np.errstate(all="ignore"):
        n = perlin_1d(st[:, 0] * scale) if dim == 1 else perlin_2d(st[:, 0] * scale, st[:, 1] * scale)
    out = np.zeros((st.shape[0], 4), dtype=F)
    out[:, 0] = n
    return out


def slope_bound(dim):
    """(L, slack): |noise(p) - noise(q)| <= L |p - q| along one axis + slack, for p and q anywhere (in one cell or in neighbouring ones).
    Inside a cell the value is lerp(g0, g1, fade(t)) of corner gradients g: |d/dt| <= max |dg/dt| + max fade' * max |g1 - g0|, fade' <= 15/8 (at
    t = 1/2). 1D: g = +-(1..8) t, so |dg/dt| <= 8 and |g| <= 8: L = 8 + 15/8 * 16. 2D: g = +-x +- 2y or +-y +- 2x over [-1, 1]^2, so |dg| <= 2 and
    |g| <= 3: L = 2 + 15/8 * 6. The function is continuous across a lattice line only because both cells hash the shared corners alike -- which is
    what the property tests. slack: the float32 evaluation, at most some 32 roundings of values no larger than max |g|."""
    gmax, dmax = (8.0, 8.0) if dim == 1 else (3.0, 2.0)
    return dmax + 15.0 / 8.0 * 2.0 * gmax, 32.0 * 2.0 ** -24 * gmax


# ---------------------------------------------------------------------------------------------- math
def math_apply(op, a, b, pow_fn=None):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    with np.errstate(all="ignore"):
        if op == 0: return a + b  # noqa: E701
        if op == 1: return a - b  # noqa: E701
        if op == 2: return a * b  # noqa: E701
        if op == 3: return a / b  # noqa: E701
        if op == 4: return np.asarray(pow_fn(a, b), dtype=F)  # noqa: E701
        if op == 5: return np.where(b < a, b, a)  # noqa: E701  (a NaN in b yields a)
        if op == 6: return np.where(a < b, b, a)  # noqa: E701
    raise ValueError(op)


def math_node(op, a, b, bc, pow_fn=None):
    """a, b (n, 4); bc bit 0: a is a scalar, bit 1: b is. Two scalars: (op(a.x, b.x), 0, 0, 0). Otherwise xyz component-wise with the scalar's .x
    broadcast, w from the first operand that is not a scalar."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    out = np.zeros(a.shape, dtype=F)
    sa, sb = bool(bc & 1), bool(bc & 2)
    if sa and sb:
        out[:, 0] = math_apply(op, a[:, 0], b[:, 0], pow_fn)
        return out
    for c in range(3):
        out[:, c] = math_apply(op, a[:, 0] if sa else a[:, c], b[:, 0] if sb else b[:, c], pow_fn)
    out[:, 3] = b[:, 3] if sa else a[:, 3]
    return out


def mapping_point(a, loc, sc):
    """node_mapping, type point: (a * sc + loc, 0), two roundings per component (the operand the tests build their varying vectors with)."""
    a = np.asarray(a, dtype=F)
    out = np.zeros(a.shape, dtype=F)
    with np.errstate(all="ignore"):
        for c in range(3):
            out[:, c] = a[:, c] * F(sc[c]) + F(loc[c])
    return out


def texcoords(uv):
    uv = np.asarray(uv, dtype=F)
    out = np.zeros((uv.shape[0], 4), dtype=F)
    out[:, :2] = uv
    return out


def bits_equal(a, b):
    """Bit equality, except that any NaN equals any NaN (a payload is not part of the definition)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (a.view(U) == b.view(U)) | (np.isnan(a) & np.isnan(b))
