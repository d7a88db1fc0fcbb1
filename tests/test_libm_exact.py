"""The device primitives every "bit-equal to the CPU path" claim rests on, each tested as its own unit.

csrc/libm_exact.hpp restates glibc's expf / atanf / sinf / cosf / atan2f and a correctly rounded division by a constant
(lm::fdiv_const); device_util.hpp::acos_abs_greater decides computePairFeatures' "switch p1 and p2"; fpfh.hip's certified
SPFH bins budget an error for their polynomial arc tangent (atan2_fast) and for v_rsq_f32 / v_rcp_f32.  The CPU tests prove
the restatements as the host compiles them (scripts/libm_sweep.cpp, tests/host_libm/fdiv_host.cpp); the GPU tests hold the
device build -- a different program -- against the host's libm (the oracle's mo_libm_eval), numpy's IEEE float32 division and
float64 references through the test hook mm3d_debug_libm (include/mm3d.h), argument by argument, on the arguments where each
primitive can go wrong."""
import ctypes as C
import ctypes.util
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 24
U = 2.0 ** -24
GXX_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]


# ---- argument sets ------------------------------------------------------------------------------------------------------
def bits_to_f32(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def fbits(v):
    """The bit pattern of one float32, as an int."""
    return int(np.float32(v).view(np.uint32))


def windows(centres, half=4096, both_signs=True):
    """Every float within +-half ulps of each centre (bit patterns; the sign bit added as well with both_signs)."""
    out = []
    for c in centres:
        b = np.arange(int(c) - half, int(c) + half + 1, dtype=np.int64)
        b = b[(b >= 0) & (b < 0x80000000)]
        out.append(b)
        if both_signs:
            out.append(b | 0x80000000)
    return bits_to_f32(np.concatenate(out).astype(np.uint32))


def sift_sigma_sqr():
    """Every sigma_sqr detectKeypoints(SIFT) divides by for min_scale in {0.05, 0.1, 0.2, 0.5, 1}, octaves 0-2, 6 scales: the
    host's float arithmetic of sift.hip (scale = (float)min_scale, doubled per octave; powf from the C library)."""
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype = C.c_float
    libm.powf.argtypes = [C.c_float, C.c_float]
    out = []
    for ms in (0.05, 0.1, 0.2, 0.5, 1.0):
        scale = np.float32(ms)
        for _ in range(3):
            for i in range(6):
                s = np.float32(scale * np.float32(libm.powf(2.0, float(np.float32((np.float32(i) - np.float32(1.0)) / np.float32(3.0))))))
                out.append(np.float32(libm.powf(float(s), 2.0)))
            scale = np.float32(scale * np.float32(2.0))
    return np.array(out, dtype=np.float32)


def fdiv_sift_arguments(per_divisor=4096, n_random=10_000, per_random=512, seed=7):
    """(x, y) for the SIFT weights' -0.5 d2 / sigma_sqr: x over the binades of [-4.5 y, 0] (log-uniform down to 2^-140 y, so
    that the tiny quotients below the promised range are there too), plus +-64-ulp windows around -4.5 y, -y, -y / 2 and every
    power of two in the range, plus the hard cases of fdiv_hard_numerators; y every sigma_sqr of sift_sigma_sqr() and n_random
    random divisors of their range."""
    rng = np.random.default_rng(seed)
    sig = sift_sigma_sqr()
    rand_y = np.exp(rng.uniform(np.log(float(sig.min()) * 0.5), np.log(float(sig.max()) * 2.0), n_random)).astype(np.float32)
    xs, ys = [], []
    for y, k in [(float(v), per_divisor) for v in sig] + [(float(v), per_random) for v in rand_y]:
        top = np.float32(4.5) * np.float32(y)
        mag = np.exp2(rng.uniform(np.log2(float(top)) - 140.0, np.log2(float(top)), k)).astype(np.float32)
        cen = [float(top), y, y * 0.5] + [2.0 ** e for e in range(int(np.log2(float(top))) - 20, int(np.log2(float(top))) + 1)]
        cen = f32_bits(np.array(cen, dtype=np.float32)).astype(np.int64)
        win = (cen[:, None] + np.arange(-64, 65)[None, :]).ravel()
        hard = fdiv_hard_numerators(y, range(-90, 1)) if k == per_divisor else fdiv_hard_numerators(y, range(-30, 1), rs=(-3, -1, 1, 3))
        x = -np.concatenate([mag, bits_to_f32(win.astype(np.uint32)), hard.astype(np.float32)])
        x = x[(x >= -top) & (x <= 0)]
        xs.append(x)
        ys.append(np.full(len(x), y, dtype=np.float32))
    return np.concatenate(xs).astype(np.float32), np.concatenate(ys).astype(np.float32)


def fdiv_hard_numerators(y, shifts, rs=tuple(range(-15, 16, 2))):
    """Numerators whose quotient by y lies within a tiny fraction of an ulp of the MIDPOINT between two floats -- the only
    quotients a faithful (one Newton step) division rounds the wrong way.  With y = Y 2^e (Y odd) and M = r / Y mod 2^25
    (r odd and small), X = (Y M - r) / 2^25 is an integer below 2^24 and X / Y = M / 2^25 - r / (Y 2^25): M odd in
    [2^24, 2^25) makes M / 2^25 a midpoint, and X / Y misses it by |r| / (2 Y) ulp.  Every power-of-two scaling keeps that."""
    yb = fbits(y)
    Y, e = (yb & 0x7fffff) | 0x800000, ((yb >> 23) & 0xff) - 150
    while Y % 2 == 0:
        Y //= 2
        e += 1
    K = 1 << 25
    inv = Y
    for _ in range(6):                                    # Newton's iteration for 1 / Y mod 2^25
        inv = inv * (2 - Y * inv) % K
    xs = []
    for r in rs:
        M = r * inv % K
        if M < (1 << 24):
            continue
        X = (Y * M - r) >> 25
        if X <= 0:
            continue
        xs += [float(X) * 2.0 ** (e + j) for j in shifts]
    return np.array(xs, dtype=np.float64)


def fdiv_promised(x, y):
    """Where the header promises the correctly rounded quotient on the SIFT range: |x| >= 2^-96 y (below it the remainders
    underflow and the callers rely on expf(q) == 1.0f instead -- sift.hip::k_sift_dog_lds)."""
    return np.abs(x.astype(np.float64)) >= 2.0 ** -96 * y.astype(np.float64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def report_mismatch(name, args, got, want):
    bad = np.flatnonzero(~same_bits(got, want))
    if len(bad) == 0:
        return ""
    i = bad[0]
    a = ", ".join(f"{float(v[i])!r} (0x{int(np.float32(v[i]).view(np.uint32)):08x})" for v in args)
    return f"{name}: {len(bad)} of {len(got)} differ, e.g. ({a}) -> {float(got[i])!r} vs {float(want[i])!r}"


# ---- CPU: the restatements as the host compiles them ----------------------------------------------------------------------
def _gxx(tmp_path, src, out, extra):
    cmd = ["g++"] + GXX_FLAGS + [os.path.join(ROOT, src), "-o", str(tmp_path / out)] + extra
    subprocess.check_call(cmd, timeout=300)
    return str(tmp_path / out)


def test_libm_sweep_host_restatements_match_the_host_libm(tmp_path):
    """scripts/libm_sweep.cpp at a stride of 1021: every restated function (atan2f on ~4 M pairs plus its specials) gives the
    host libm's bits on every argument it checks."""
    exe = _gxx(tmp_path, "scripts/libm_sweep.cpp", "libm_sweep", ["-fopenmp", "-lm"])
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
    r = subprocess.run([exe, "1021"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {m.group(1): (int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"^(\w+) checked (\d+) mismatches (\d+)", r.stdout, re.M)}
    print(r.stdout)
    assert sorted(lines) == ["atan2f", "atanf", "cosf", "expf", "sinf"], r.stdout
    for name, (checked, bad) in lines.items():
        assert checked >= 1_000_000, f"{name}: only {checked} arguments checked"
        assert bad == 0, f"{name}: {bad} mismatches\n{r.stdout}"


@pytest.fixture(scope="module")
def host_fdiv(tmp_path_factory):
    d = tmp_path_factory.mktemp("fdiv")
    so = _gxx(d, "tests/host_libm/fdiv_host.cpp", "libfdiv_host.so", ["-shared", "-fPIC"])
    L = C.CDLL(so)
    L.fdiv_const_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]

    def run(x, y, rcp=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty_like(x)
        r = None if rcp is None else np.ascontiguousarray(rcp, dtype=np.float32)
        L.fdiv_const_eval(x.ctypes.data, y.ctypes.data, None if r is None else r.ctypes.data, len(x), out.ctypes.data)
        return out
    return run


def test_host_fdiv_const_is_ieee_division_on_every_intensity(host_fdiv):
    """intensity_of's (299 r + 587 g + 114 b) / 1000: every numerator 0 ... 255 000 with the reciprocal the kernels pass
    (0.001f, which is RN(1 / 1000) -- the constant tested is the one in the source)."""
    assert np.float32(1.0 / 1000.0) == np.float32(0.001)
    x = np.arange(0, 255_001, dtype=np.float32)
    y = np.full(len(x), 1000.0, dtype=np.float32)
    got = host_fdiv(x, y, np.full(len(x), 0.001, dtype=np.float32))
    want = x / y
    msg = report_mismatch("fdiv_const(n, 1000)", [x, y], got, want)
    assert not msg, msg


def test_host_fdiv_const_is_ieee_division_on_the_sift_weights(host_fdiv):
    """-0.5 d2 / sigma_sqr: bits of IEEE float division wherever the header promises them, and below that expf of both
    quotients is 1.0f (what the kernel relies on there)."""
    x, y = fdiv_sift_arguments()
    got = host_fdiv(x, y)
    want = x / y
    ok = fdiv_promised(x, y)
    print(f"fdiv_const (host): {len(x)} quotients, {int(ok.sum())} in the promised range")
    msg = report_mismatch("fdiv_const", [x[ok], y[ok]], got[ok], want[ok])
    assert not msg, msg
    tiny = ~ok
    assert tiny.sum() > 1000
    assert np.all(np.exp(got[tiny].astype(np.float64)).astype(np.float32) == 1.0)
    assert np.all(np.exp(want[tiny].astype(np.float64)).astype(np.float32) == 1.0)


# ---- GPU: the device build against the host -----------------------------------------------------------------------------
def dev_eval(ctx, mm, fn, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float32)
    out = np.empty_like(x)
    for a in range(0, len(x), CHUNK):
        b = min(a + CHUNK, len(x))
        xp = x[a:b].ctypes.data_as(C.c_void_p)
        yp = None if y is None else y[a:b].ctypes.data_as(C.c_void_p)
        o = out[a:b]
        ctx._ck(mm.lib().mm3d_debug_libm(ctx._h, fn, xp, yp, b - a, o.ctypes.data_as(C.c_void_p)))
    return out


def host_eval(po, fn, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    for a in range(0, len(x), CHUNK):
        b = min(a + CHUNK, len(x))
        out[a:b] = po.libm_eval(fn, x[a:b], None if y is None else y[a:b])
    return out


def strided_all(stride=257):
    return bits_to_f32(np.arange(0, 1 << 32, stride, dtype=np.uint64).astype(np.uint32))


ATANF_SWITCHES = [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000]
EXPF_SWITCHES = [0x42b00000, fbits(88.72283172607421875), fbits(103.972076416015625)]
# sin/cos: 2^-12, the top-12-bit pi/4 test (0x3f4xxxxx) and pi/4 itself, and 120 (the end of the restated range)
SINCOS_SWITCHES = [0x39800000, 0x3f400000, 0x3f490fdb, 0x3f500000, 0x42f00000]


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name,switches", [(0, "expf", EXPF_SWITCHES), (1, "atanf", ATANF_SWITCHES),
                                              (2, "sinf", SINCOS_SWITCHES), (3, "cosf", SINCOS_SWITCHES)])
def test_device_libm_matches_the_host_libm(ctx, mm, po, fn, name, switches):
    """All 2^32 bit patterns at a stride of 257 plus every float within 4 k ulps of each range switch.  sinf / cosf are
    restated for |x| < 120 only (the callers' arguments are angles in [-pi, pi]; beyond it the device calls ocml), so their
    arguments are restricted to that range."""
    x = np.concatenate([strided_all(257), windows(switches)])
    if fn in (2, 3):
        x = x[np.abs(x) < 120.0]
    got = dev_eval(ctx, mm, fn, x)
    want = host_eval(po, fn, x)
    print(f"{name}: {len(x)} arguments")
    msg = report_mismatch(name, [x], got, want)
    assert not msg, msg


def atan2_arguments(seed=11):
    rng = np.random.default_rng(seed)
    ys, xs = [], []
    # a lattice of exponents x mantissas, all four quadrants
    mant = np.array([1.0, 1.0000001, 1.25, 1.5, 1.75, 1.9999999], dtype=np.float64)
    exps = np.arange(-149, 128, 4)
    v = (mant[None, :] * np.exp2(exps)[:, None]).ravel().astype(np.float32)
    v = v[np.isfinite(v) & (v != 0)]
    v = np.concatenate([v, -v])
    Y, X = np.meshgrid(v, v, indexing="ij")
    ys.append(Y.ravel()); xs.append(X.ravel())
    # every zero / inf / NaN / x == 1 combination (with ordinary and extreme partners)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -2.0, 1e-45, -1e-45, 1.17e-38, 3.4e38, -3.4e38, 1e-30, 7.0],
                  dtype=np.float32)
    Y, X = np.meshgrid(sp, sp, indexing="ij")
    ys.append(Y.ravel()); xs.append(X.ravel())
    # |y / x| around 2^+-60 (the exponent difference k = 59, 60, 61 and its negatives), every sign
    n = 1 << 20
    ex = rng.integers(-60, 60, n)
    k = rng.choice([-61, -60, -59, 59, 60, 61], n)
    x = (rng.uniform(1, 2, n) * np.exp2(ex)).astype(np.float32)
    y = (rng.uniform(1, 2, n) * np.exp2(ex + k)).astype(np.float32)
    sx, sy = rng.choice([-1, 1], n).astype(np.float32), rng.choice([-1, 1], n).astype(np.float32)
    ys.append(y * sy); xs.append(x * sx)
    # the callers' domain: dense pairs in [-1.1, 1.1]^2, and dense near the axes and the diagonals
    n = 1 << 23
    ys.append(rng.uniform(-1.1, 1.1, n).astype(np.float32)); xs.append(rng.uniform(-1.1, 1.1, n).astype(np.float32))
    n = 1 << 21
    a = rng.uniform(-1.1, 1.1, n).astype(np.float32)
    b = (a * np.exp2(rng.uniform(-30, 0, n))).astype(np.float32)
    ys += [b, a, a, -a]; xs += [a, b, a * np.float32(1.0000001), a]
    return np.concatenate(ys).astype(np.float32), np.concatenate(xs).astype(np.float32)


@pytest.mark.gpu
def test_device_atan2f_matches_the_host_libm(ctx, mm, po):
    """atan2f(y, x) on a lattice of exponents x mantissas in all four quadrants, every special operand combination, |y / x|
    around 2^+-60 and dense pairs of the callers' domain [-1.1, 1.1]^2."""
    y, x = atan2_arguments()
    got = dev_eval(ctx, mm, 4, x, y)
    want = host_eval(po, 4, x, y)
    print(f"atan2f: {len(x)} argument pairs")
    msg = report_mismatch("atan2f", [y, x], got, want)
    assert not msg, msg


@pytest.mark.gpu
def test_sift_expf_with_the_lds_table_matches_the_host_expf(ctx, mm, po):
    """fn 6, expf as the SIFT kernels call it (LDS table, no range checks): every 13th float of [-4.5, 0] and every float of the
    binades [-1, -0.5) and [-4, -2), against the host's expf (fn 0's reference)."""
    lo, hi = 0x80000000, fbits(-4.5)
    b = [np.arange(lo, hi + 1, 13, dtype=np.uint64)]
    for top in (-0.5, -2.0):
        s = fbits(top)
        b.append(np.arange(s, s + (1 << 23), dtype=np.uint64))
    x = bits_to_f32(np.concatenate(b).astype(np.uint32))
    got = dev_eval(ctx, mm, 6, x)
    want = host_eval(po, 0, x)
    print(f"expf (LDS table): {len(x)} arguments")
    msg = report_mismatch("expf_glibc_t<false>", [x], got, want)
    assert not msg, msg


@pytest.mark.gpu
def test_device_fdiv_const_is_ieee_division(ctx, mm):
    """fn 7 on the SIFT weights' divisions (fdiv_sift_arguments) and the intensities' / 1000: the bits of numpy's IEEE float32
    division wherever the header promises them; below that range expf of both quotients is 1.0f."""
    x, y = fdiv_sift_arguments()
    xi = np.arange(0, 255_001, dtype=np.float32)
    x = np.concatenate([x, xi])
    y = np.concatenate([y, np.full(len(xi), 1000.0, dtype=np.float32)])
    got = dev_eval(ctx, mm, 7, x, y)
    want = x / y
    ok = fdiv_promised(x, y)
    print(f"fdiv_const: {len(x)} quotients, {int(ok.sum())} in the promised range")
    msg = report_mismatch("fdiv_const", [x[ok], y[ok]], got[ok], want[ok])
    assert not msg, msg
    tiny = ~ok
    assert tiny.sum() > 1000
    assert np.all(np.exp(got[tiny].astype(np.float64)).astype(np.float32) == 1.0)
    assert np.all(np.exp(want[tiny].astype(np.float64)).astype(np.float32) == 1.0)


def acos_arguments(seed=5):
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    n = 6_000_000
    xs.append(rng.uniform(-1.01, 1.01, n)); ys.append(rng.uniform(-1.01, 1.01, n))
    # adjacent floats from 1 down to 2^-70, both orders and the equal pair, mixed signs
    m = 1_000_000
    base = f32_bits((rng.uniform(1, 2, m) * np.exp2(rng.integers(-70, 1, m))).astype(np.float32))
    base = np.minimum(base, fbits(1.0) - 1)
    a, b = bits_to_f32(base), bits_to_f32(base + 1)
    sg = rng.choice([-1.0, 1.0], (2, m))
    xs += [a * sg[0], b * sg[0], a]; ys += [b * sg[1], a * sg[1], a * sg[1]]
    # both below 2^-28 (the double arc cosines can tie there): log-uniform, and adjacent pairs
    lo = f32_bits((rng.uniform(1, 2, m) * np.exp2(rng.integers(-149, -28, m))).astype(np.float32))
    xs += [bits_to_f32(lo), bits_to_f32(lo)]
    ys += [bits_to_f32(f32_bits((rng.uniform(1, 2, m) * np.exp2(rng.integers(-149, -28, m))).astype(np.float32))), bits_to_f32(lo + 1)]
    # 1 and 1 + ulp, +-0, subnormals, NaN, infinities: every combination
    sp = np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), 0.0, -0.0, 1e-45, 3e-39,
                   2.0 ** -28, np.nextafter(np.float32(2.0 ** -28), np.float32(0)), np.nan, np.inf, -np.inf, 0.5], dtype=np.float32)
    sp = np.concatenate([sp, -sp])
    Y, X = np.meshgrid(sp, sp, indexing="ij")
    xs.append(X.ravel()); ys.append(Y.ravel())
    return (np.concatenate([np.asarray(v, dtype=np.float32) for v in xs]),
            np.concatenate([np.asarray(v, dtype=np.float32) for v in ys]))


@pytest.mark.gpu
def test_acos_abs_greater_matches_the_oracle(ctx, mm, po):
    """fn 8 against the oracle's own expression acos(fabs(x)) > acos(fabs(y)) (mo_libm_eval fn 5) on > 10^7 pairs: random in
    [-1.01, 1.01]^2, adjacent floats from 1 down to 2^-70, pairs below 2^-28, and 1, 1 + ulp, +-0, subnormals, NaN."""
    x, y = acos_arguments()
    assert len(x) >= 10_000_000
    got = dev_eval(ctx, mm, 8, x, y)
    want = host_eval(po, 5, x, y)
    print(f"acos_abs_greater: {len(x)} pairs, {int(want.sum())} true")
    msg = report_mismatch("acos_abs_greater", [x, y], got, want)
    assert not msg, msg


@pytest.mark.gpu
def test_atan2_fast_is_within_its_budget(ctx, mm):
    """fn 9, the polynomial arc tangent of pair_bins_fast: within the 10 u (u = 2^-24, absolute) the bound derivation in
    fpfh.hip budgets, against float64 atan2, for rho = |(x, y)| in [1e-3, 1.05], every quadrant, both axes and the diagonals."""
    rng = np.random.default_rng(3)
    n = 1 << 23
    rho = np.exp(rng.uniform(np.log(1e-3), np.log(1.05), n))
    th = rng.uniform(-np.pi, np.pi, n)
    x, y = (rho * np.cos(th)).astype(np.float32), (rho * np.sin(th)).astype(np.float32)
    m = 1 << 18
    r = np.exp(rng.uniform(np.log(1e-3), np.log(1.05), m)).astype(np.float32)
    z = np.zeros(m, dtype=np.float32)
    xs = [x, r, -r, z, z, -r, r, -r, r, -r, r * np.float32(1.0000001)]
    ys = [y, z, z, r, -r, -z, -z, r, r, -r, r]
    x, y = np.concatenate(xs), np.concatenate(ys)
    got = dev_eval(ctx, mm, 9, x, y).astype(np.float64)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    err = np.abs(got - want) / U
    i = int(np.argmax(err))
    print(f"atan2_fast: {len(x)} pairs, worst {err[i]:.2f} u at (y, x) = ({float(y[i])!r}, {float(x[i])!r})")
    assert err[i] <= 10.0


@pytest.mark.gpu
@pytest.mark.parametrize("fn,name,lo,hi", [(10, "v_rsq_f32", 1.0, 4.0), (11, "v_rcp_f32", 1.0, 2.0)])
def test_rsq_rcp_within_one_ulp(ctx, mm, fn, name, lo, hi):
    """fn 10 / 11, the raw v_rsq_f32 and v_rcp_f32 pair_bins_fast budgets 1 ulp for: every float of [1, 4) (rsq, two binades:
    the result's pattern repeats with period 4) or [1, 2) (rcp), plus every 257th normal float whose result is normal too,
    against float64."""
    b0, b1 = fbits(lo), fbits(hi)
    full = np.arange(b0, b1, dtype=np.uint32)
    top = 0x7f7fffff if fn == 10 else 0x7e800000           # rcp: 1 / x stays normal below 2^126
    x = bits_to_f32(np.concatenate([full, np.arange(0x00800000, top, 257, dtype=np.uint32)]))
    got = dev_eval(ctx, mm, fn, x).astype(np.float64)
    xd = x.astype(np.float64)
    want = 1.0 / np.sqrt(xd) if fn == 10 else 1.0 / xd
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    i = int(np.argmax(err))
    print(f"{name}: {len(x)} arguments, worst {err[i]:.3f} ulp at x = {float(x[i])!r}")
    assert err[i] <= 1.0
