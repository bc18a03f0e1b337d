"""float64 model of the on-device channel generators (csrc/vaeq_gen.hip, csrc/vaeq_gen_fused.h): numpy only, float64 / complex128 throughout,
independent of the native library -- the yardstick of test_generator_envelope_gpu.py, itself checked on the CPU by test_ref_generator_host.py.

Every random value of a frame is a pure function of (key, frame, run, stream, pol, index) through Philox4x32-10:

    counter = (index >> 1, run, frame, stream * 2 + pol),  key = the 64-bit stream key as two 32-bit words (low, high)

``stream`` is STREAM_SYMBOLS for the PCS symbols (index = symbol number n; words (x, y) give I / Q of even n, (z, w) of odd n) and STREAM_NOISE
for the AWGN (index = sample number s; words (x, y) give radius / angle of even s, (z, w) of odd s).  Runs are generated in blocks of
STREAM_BLOCK: run r draws with the key mix_seed(seed, r - r % STREAM_BLOCK) and the run counter r % STREAM_BLOCK.

The uniforms are the kernels' float32 values bit for bit (u01); everything after them is float64.  Note that u01 is ((w >> 8) + 0.5) * 2^-24
evaluated in float32: above 2^23 the half is absorbed (round to even), so u lies in [2^-25, 1] and reaches exactly 1.0 for the topmost
word (probability 2^-24).  The models below replicate that: a radius of 0 for the noise, the top level for a symbol."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
STREAM_SYMBOLS, STREAM_NOISE = 0, 1
STREAM_BLOCK = 8192
PULSE_SPAN = 8


# ------------------------------------------------------------------ random streams
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """numpy Philox4x32-10 (Salmon et al.), vectorised over uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def u01(v):
    """The kernels' uniform of a 32-bit word, in float32 arithmetic like theirs (see the module docstring for its range)."""
    return ((np.asarray(v, np.uint64) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def mix_seed(seed, r0):
    """Key of the stream block that starts at run r0."""
    return (int(seed) * 0x9E3779B97F4A7C15 + int(r0) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def block_key_and_run(seed, r):
    """(key, run counter) of run r of a batch: blocks of STREAM_BLOCK runs differ in the key, runs inside a block in the counter word."""
    r0 = int(r) - int(r) % STREAM_BLOCK
    return mix_seed(seed, r0), int(r) - r0


def stream_counters(stream, frame, run, pol, index):
    """Philox counter words (c0, c1, c2, c3) of the values with the given indices (symbol numbers / sample numbers) of one stream."""
    idx = np.asarray(index, np.uint64)
    return idx >> np.uint64(1), np.full_like(idx, run), np.full_like(idx, frame), np.full_like(idx, stream * 2 + pol)


def counter_tuples(stream, key, frame, run, pol, index):
    """The distinct (c0, c1, c2, c3, k0, k1) tuples symbols() / noise() feed to Philox for these indices, as a set."""
    c = stream_counters(stream, frame, run, pol, index)
    k0, k1 = int(key) & 0xFFFFFFFF, int(key) >> 32
    return {(int(a), int(b), int(c_), int(d), k0, k1) for a, b, c_, d in zip(*c)}


def _words(stream, key, frame, run, pol, index):
    """Per index: the two 32-bit words that serve it -- (x, y) for an even index, (z, w) for an odd one."""
    idx = np.asarray(index, np.uint64)
    x, y, z, w = philox4x32_10(*stream_counters(stream, frame, run, pol, idx), int(key) & 0xFFFFFFFF, int(key) >> 32)
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd, z, x), np.where(odd, w, y)


def cdf_table(P):
    """The float32 cumulative table the kernels are given: cumulated in float64, then rounded."""
    return np.cumsum(np.asarray(P, np.float64), axis=-1).astype(np.float32)


def levels(u, cdf_f32):
    """Inverse CDF like draw_symbol_pair: the number of thresholds cdf[0 .. n_lev-2] that u reaches.  Never n_lev, whatever cdf[-1] is."""
    cdf = np.asarray(cdf_f32, np.float32)
    return (np.asarray(u, np.float32)[..., None] >= cdf[:-1]).sum(-1)


def symbols(key, frame, run, pol, n, cdf_f32):
    """Level indices [2 (I, Q), len(n)] of the symbols with numbers n of (run, pol)."""
    a, b = _words(STREAM_SYMBOLS, key, frame, run, pol, n)
    return np.stack([levels(u01(a), cdf_f32), levels(u01(b), cdf_f32)])


def noise(key, frame, run, pol, n_samples):
    """Unit-variance (per real component) complex AWGN of samples 0 .. n_samples-1 of (run, pol): Box-Muller on the stream's words, in
    float64.  The caller scales by sigma."""
    a, b = _words(STREAM_NOISE, key, frame, run, pol, np.arange(n_samples))
    rad = np.sqrt(-2.0 * np.log(u01(a).astype(np.float64)))
    ang = 2.0 * np.pi * u01(b).astype(np.float64)
    return rad * (np.cos(ang) + 1j * np.sin(ang))


# ------------------------------------------------------------------ signal chain
def awgn_clean(sym, g, sps):
    """np.convolve 'valid' of the zero-stuffed symbols with the combined pulse g (the complex64 taps the kernel is given), complex128."""
    sym = np.asarray(sym, np.complex128)
    up = np.zeros(sps * (len(sym) - 1) + 1, np.complex128)
    up[::sps] = sym
    return np.convolve(up, np.asarray(g).astype(np.complex128), mode="valid")


def fiber_matrix(freq, tau_pmd, phiIQ, theta):
    """H(f) = R^T diag(e^{j pi tau f}, e^{-j pi tau f}) R with the IQ phase folded into R, complex128."""
    d = np.exp(1j * np.pi * float(tau_pmd) * freq)
    c, s = np.cos(float(theta)), np.sin(float(theta))
    e = np.exp(-1j * np.asarray(phiIQ).astype(np.complex128))
    R = ((c * e[0], s * e[0]), (-s * e[1], c * e[1]))
    RT = ((c * e[0], -s * e[0]), (s * e[1], c * e[1]))
    di = 1 / d
    return [[RT[a][0] * d * R[0][b] + RT[a][1] * di * R[1][b] for b in range(2)] for a in range(2)]


def dp_clean(sym, g, sps, N, symb_rate, tau_cd, tau_pmd, phiIQ, theta, Lrow=None):
    """Noise-free DP frame: sym[2, N_conv] complex -> (clean[2, sps N] after the fibre, pre[2, Ls] before it).  Pulse shaping per
    polarisation, zero padding to Lrow (None: Ls, the circular 'exact' frame), fibre matrix and CD phase on fftfreq(Lrow), inverse FFT."""
    pre = np.stack([awgn_clean(sym[p], g, sps) for p in range(2)])
    Ls = pre.shape[1]
    Lrow = Ls if Lrow is None else int(Lrow)
    row = np.zeros((2, Lrow), np.complex128)
    row[:, :Ls] = pre
    spec = np.fft.fft(row, axis=1)
    freq = np.fft.fftfreq(Lrow, 1 / (float(symb_rate) * sps))
    cd = np.exp(1j * 2 * (np.pi * freq) ** 2 * float(tau_cd))
    H = fiber_matrix(freq, tau_pmd, phiIQ, theta)
    out = np.stack([(H[0][0] * spec[0] + H[0][1] * spec[1]) * cd, (H[1][0] * spec[0] + H[1][1] * spec[1]) * cd])
    return np.fft.ifft(out, axis=1)[:, :sps * N], pre


def sigma(clean_pre, Ls, sps, snr_db):
    """sqrt(mean |x|^2 sps / 2 / 10^(SNR/10)) over the first Ls samples before the fibre (all polarisations)."""
    x = np.asarray(clean_pre)[..., :Ls]
    return float(np.sqrt(np.mean(np.abs(x) ** 2) * sps / 2 / 10 ** (float(snr_db) / 10)))


# ------------------------------------------------------------------ whole frames of one run
def awgn_run(key, frame, run, amps32, cdf_f32, g, sps, N, N_conv, ref_offset):
    """(levels[2, N_conv], clean[Ls], unit noise[sps N]) of one run of the single-polarisation generator."""
    lev = symbols(key, frame, run, 0, np.arange(N_conv), cdf_f32)
    a = np.asarray(amps32, np.float32).astype(np.float64)[lev]
    return lev, awgn_clean(a[0] + 1j * a[1], g, sps), noise(key, frame, run, 0, sps * N)


def dp_run(key, frame, run, amps32, cdf_f32, g, sps, N, N_conv, symb_rate, tau_cd, tau_pmd, phiIQ, theta, Lrow=None):
    """(levels[2 pol, 2, N_conv], clean[2, sps N], pre[2, Ls], unit noise[2, sps N]) of one run of the dual-polarisation generator."""
    lev = np.stack([symbols(key, frame, run, p, np.arange(N_conv), cdf_f32) for p in range(2)])
    a = np.asarray(amps32, np.float32).astype(np.float64)[lev]
    clean, pre = dp_clean(a[:, 0] + 1j * a[:, 1], g, sps, N, symb_rate, tau_cd, tau_pmd, phiIQ, theta, Lrow)
    return lev, clean, pre, np.stack([noise(key, frame, run, p, sps * N) for p in range(2)])
