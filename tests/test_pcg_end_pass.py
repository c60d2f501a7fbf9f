"""The end of a pass of the independent sampler, advance(-dim) (sampler/mod.rs:168-177): the kernels' closed form
(csrc/device/drng.h pcg_end_pass, run on the host through akr_host_pcg_end_pass) against the oracle's restatement of the
reference loop, bit for bit. The closed form has one path for every 32-bit dim (no fast range, no fallback)."""
import ctypes as C

import numpy as np

from akari_render_amd import capi

C2_PASS_DIM_MAX = 5504  # the largest dim a C2 pass can reach


def edge_dims():
    """Every power of two +- 1 up to 2^32, and 2^32 - 1."""
    out = set()
    for k in range(33):
        out.update(d for d in (2**k - 1, 2**k, 2**k + 1) if 0 <= d < 2**32)
    out.add(2**32 - 1)
    return sorted(out)


def random_generators(rng, n):
    """n random (state, inc) with odd and even inc alternating (the loop is defined for either)."""
    state = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    inc = (inc & ~np.uint64(1)) | (np.arange(n, dtype=np.uint64) & np.uint64(1))
    return state, inc


def oracle_end_pass(oracle_lib, state, inc, dim):
    st = C.c_uint64(int(state))
    oracle_lib.or_kat_pcg32_advance(C.byref(st), C.c_uint64(int(inc)), C.c_int64(-int(dim)))
    return st.value


def check(oracle_lib, dims, seed):
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims, dtype=np.uint64)
    # both parities of inc for every dim
    state, inc = random_generators(rng, 2 * dims.size)
    for i, d in enumerate(np.repeat(dims, 2)):
        s, c, d = int(state[i]), int(inc[i]), int(d)
        assert capi.host_pcg_end_pass(s, c, d) == oracle_end_pass(oracle_lib, s, c, d), f"dim {d} state {s:#x} inc {c:#x}"


def test_every_dim_of_a_c2_pass(hip_lib, oracle_lib):
    check(oracle_lib, range(C2_PASS_DIM_MAX + 1), seed=11)


def test_powers_of_two_and_their_neighbours(hip_lib, oracle_lib):
    dims = edge_dims()
    assert dims[0] == 0 and dims[-1] == 2**32 - 1 and 2**16 + 1 in dims and 2**31 - 1 in dims
    check(oracle_lib, dims, seed=12)


def test_random_32_bit_dims(hip_lib, oracle_lib):
    """No fast range to step out of: 1000 random dims over the whole 32 bits, and 1000 just past 2^16 where a pass of 1024 spp gets."""
    rng = np.random.default_rng(13)
    check(oracle_lib, rng.integers(0, 2**32, size=1000, dtype=np.uint64), seed=14)
    check(oracle_lib, rng.integers(2**16, 2**18, size=1000, dtype=np.uint64), seed=15)
