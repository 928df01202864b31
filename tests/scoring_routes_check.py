"""Dense scoring and the AS-norm statistics on every route, against float64: the case tables, the seeded inputs, the route predicates
and the bars of tests/test_gpu_scoring_routes.py.  None of it needs a GPU, so tests/test_scoring_routes_host.py checks the predicates
against the sources they restate, the tables against the predicates, and the inputs against the properties the GPU test relies on.

References are float64 throughout: oracle/scoring.py::asnorm_stats on float64 inputs and A.astype(f64) @ B.astype(f64).T.

ROUTES (restated below, each with the function it restates)
  svhip_asnorm_stats   fused kernel for D in {192, 256}, top <= 256, K >= 4 top, K >= 64, 16-byte aligned operands and no option asnorm_slab
                       (asnorm_fused.hip::asnorm_fused_supported, api_asnorm.hip::svhip_asnorm_stats); everything else, and the rows
                       the fused kernel cannot decide, takes the slab path: a cohort GEMM into slabs of slab_rows rows, then one of the
                       four forms of the selection (score.hip::topk_stats_form): reg8 (K <= 2048), reg24 (K <= 6144), lds (Kp <= 37 888,
                       4 / 3 / 2 / 1 rows per workgroup) and global (longer rows, read from the slab on every pass).
  svhip_score_matrix   option score_f32mfma first; the row-streaming kernel for D in {192, 256} with 16-byte aligned operands
                       (score_h3w.hip::score_h3w_supported, api_scoring.hip::score_route); the tiled split GEMM otherwise.
  pair kernels         16-byte loads when D % 4 == 0 and E is 16-byte aligned, element loads otherwise (score.hip::pair_kernel).

BARS.  None is taken from what the kernels give.
  statistics, unit rows    top <= 256: |mu - ref| <= 1e-6, |sd - ref| <= 1e-4 ref.min() (tests/test_gpu_scoring.py); top = 1: |sd| <= 1e-6.
  statistics, integer data components in {-2 .. 2}: every score an exact integer, every partial sum below 2^24, so mu is one fp32 rounding from
                           the float64 value (6e-8 relative) and sd within 1e-6 relative.
  top > 256                the exact search adds top / 64 fp32 terms per lane and a 6-step butterfly follows: each bar above becomes
                           max(that bar, 4 (top / 64 + 6) 2^-24 max|s|) (summation_bar).
  score_matrix             tiled split GEMM 1e-6 and row-streaming kernel 2e-7 of |a||b| (tests/test_gpu_scoring.py); the tiled bar is
                           asserted on the rows inside TILED_NORM_RANGE, the range include/svhip.h states for that route.  Option
                           score_f32mfma was to meet 2e-7 as well; it gives up to 2.75e-7 at every magnitude, so its bar is twice what
                           it measured against float64 (F32MFMA_BAR).

MEASURED holds what the MI355X gave beside each bar (the GPU test prints every figure).  A record, not a bar: nothing reads it."""
import numpy as np

# ---- constants the predicates restate (tests/test_scoring_routes_host.py reads them back from the sources' text) -------------------------
TOPK_CAP = 512                        # score.hip: candidate slots per row
REG8_MAX_K, REG24_MAX_K = 256 * 8, 256 * 24           # score.hip::topk_stats_form
LDS_ROW_BUDGET = 150 * 1024           # score.hip::topk_stats_form: bytes of rows per workgroup of the LDS form
LDS_MAX_ROWS = 4
FAST_MAX_TOP = 256                    # score.hip: the threshold fast path runs for top <= 256 and K >= 4 top
FUSED_WIDTHS = (192, 256)             # asnorm_fused.hip::asnorm_fused_supported, score_h3w.hip::score_h3w_supported
FUSED_MIN_K = 64
SLAB_BYTES, SLAB_MIN_ROWS = 1 << 31, 128              # api_scoring.hip::SlabWalk::open
BIG_SCRATCH = 256 << 20               # api_scoring.hip::release_big_scratch
ERR_UNSUPPORTED = -5                  # include/svhip.h
FORMS = ("reg8", "reg24", "lds", "global")
LABEL = {f: "asnorm_topk_" + f for f in FORMS}        # api_asnorm.hip::asnorm_stats_slab


def kp(K):
    """row stride of the slab and padded row length of the selection: K rounded up to 4 (asnorm_stats_slab's ldk, topk_stats_form's Kp)"""
    return (K + 3) & ~3


def topk_form(K, ld=None, aligned=True):
    """score.hip::topk_stats_form -> (form, rows_per_wg)"""
    ld = kp(K) if ld is None else ld
    if ld % 4 == 0 and aligned and K <= REG24_MAX_K:
        return ("reg8" if K <= REG8_MAX_K else "reg24"), 4
    rpw = LDS_ROW_BUDGET // ((kp(K) + TOPK_CAP) * 4)
    if rpw < 1:
        return "global", 4
    return "lds", min(rpw, LDS_MAX_ROWS)


def resolve_top(K, top):
    """api_asnorm.hip::svhip_asnorm_stats: python slice semantics of S[:top]"""
    top = K + top if top < 0 else top
    return min(top, K)


def exact_search(K, top):
    """score.hip, every form: the 32-pass search instead of the threshold fast path"""
    top = resolve_top(K, top)
    return not (top <= FAST_MAX_TOP and K >= 4 * top)


def asnorm_fused_supported(D, K, top):
    """asnorm_fused.hip::asnorm_fused_supported"""
    return D in FUSED_WIDTHS and 1 <= top <= 256 and K >= 4 * top and K >= FUSED_MIN_K


def is_aligned(*ptrs):
    """the alignment rule of every route: all operands on 16-byte boundaries"""
    return all(p % 16 == 0 for p in ptrs)


def asnorm_route(D, K, top, aligned=True, slab_option=False):
    """api_asnorm.hip::svhip_asnorm_stats on a default (not f32x3) handle"""
    return "fused" if aligned and asnorm_fused_supported(D, K, resolve_top(K, top)) and not slab_option else "slab"


def score_h3w_supported(D, Na, Nb):
    """score_h3w.hip::score_h3w_supported"""
    return D in FUSED_WIDTHS and Na > 0 and 0 < Nb < (1 << 30) and Na < (1 << 31)


def score_route(D, Na, Nb, aligned=True, f32mfma=False, tiled=False):
    """api_scoring.hip::score_route on a default handle"""
    if f32mfma:
        return "f32mfma"
    return "h3w" if not tiled and score_h3w_supported(D, Na, Nb) and aligned else "words"


def slab_rows(N, K):
    """api_scoring.hip::SlabWalk::open"""
    return min(N, max(SLAB_MIN_ROWS, SLAB_BYTES // (kp(K) * 4)))


def pair_vector_loads(D, aligned):
    """score.hip::pair_kernel"""
    return D % 4 == 0 and aligned


# ---- a. the selection kernels of the slab path -------------------------------------------------------------------------------------------
def lds_band_edges():
    """the largest Kp each rows_per_wg holds, from the restated formula: {4: 9088, 3: 12288, 2: 18688, 1: 37888}"""
    return {r: (LDS_ROW_BUDGET // (4 * r) - TOPK_CAP) & ~3 for r in (4, 3, 2, 1)}


# K on both sides of every switch, 37 888 (the last row the LDS holds) and one K that is no multiple of 4 in each LDS band
SWITCH_K = (2048, 2049, 6144, 6145, 9088, 9092, 12288, 12292, 18688, 18692, 37888)
RAGGED_K = (7001, 10001, 15002, 25003)
TOPS_FAST = (1, 200, 256)
TOPS_EXACT = lambda K: (257, K // 4 + 1, K, -1)
BEYOND_K = (37892, 50000)             # b. cohorts beyond the LDS limit
TIE_TOPS = lambda K: (200, 256, 257, K // 4 + 1)      # the tops at which the integer data must tie (top = 1, K, K - 1 sit in the thin tails)


def tops_of(K):
    return TOPS_FAST + TOPS_EXACT(K)


def _case(D, K, N, data, slab_option=False):
    return dict(id=f"{data}-D{D}-K{K}-N{N}", D=D, K=K, N=N, data=data, slab_option=slab_option)


# N = 11 leaves a partly filled last workgroup for rows_per_wg = 2, 3 and 4 and for the 4 rows of the register forms (9 would fill
# the last workgroup of three rows)
SELECT_CASES = tuple(
    [_case(64, K, 11, data) for K in SWITCH_K + RAGGED_K for data in ("unit", "int")]
    + [_case(D, K, 33, "unit") for D in (320, 512) for K in (2049, 6145, 9092, 37888)]
    + [_case(192, K, 130, "unit", slab_option=True) for K in (2049, 6145, 12292)]
)
ODD_K = 7000                          # the two shapes of test_fused_asnorm_hands_odd_embeddings_to_the_slab_path, in the LDS kernel
# (the integer case pins "ties at the threshold counted exactly" in the form that reads the slab, too)
BEYOND_CASES = tuple([_case(512, K, 11, "unit") for K in BEYOND_K] + [_case(192, K, 130, "unit_zero") for K in BEYOND_K]
                     + [_case(64, BEYOND_K[0], 11, "int")])
TWO_SLAB = dict(K=37888, D=64, extra=5, top=200)      # c. N = slab_rows + 5


def unit_rows(rng, n, D):
    x = rng.standard_normal((n, D)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def seed_of(case):
    return case["D"] * 1000003 + case["K"] * 7 + case["N"] + {"unit": 0, "int": 1, "unit_zero": 2}[case["data"]]


def inputs(case):
    """(E, cohort) float32 of a case.  unit: Gaussian rows of norm 1 with two duplicated cohort rows; unit_zero: the same with one all-zero
    embedding (every score equal: the fused kernel flags it); int: components in {-2 .. 2}, scores exact integers with many ties."""
    rng = np.random.Generator(np.random.PCG64(seed_of(case)))
    D, K, N = case["D"], case["K"], case["N"]
    if case["data"] == "int":
        return rng.integers(-2, 3, (N, D)).astype(np.float32), rng.integers(-2, 3, (K, D)).astype(np.float32)
    E, C = unit_rows(rng, N, D), unit_rows(rng, K, D)
    C[3] = C[5]
    C[K - 1] = C[K // 2]
    if case["data"] == "unit_zero":
        E[N // 2] = 0.0
    return E, C


def odd_inputs(K=ODD_K, D=192, N=64):
    """a 700-row near-duplicate upper tail and an all-zero embedding, as test_fused_asnorm_hands_odd_embeddings_to_the_slab_path builds them"""
    rng = np.random.Generator(np.random.PCG64(77))
    C, E = unit_rows(rng, K, D), unit_rows(rng, N, D)
    hot = C[0].copy()
    C[100:800] = hot + rng.standard_normal((700, D)).astype(np.float32) * 0.02
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    E[10] = hot
    E[11] = hot + 0.05 * E[11]
    E[11] /= np.linalg.norm(E[11])
    E[12] = 0.0
    return E, C


class Reference:
    """the float64 scores of a case, sorted once, best first; stats(top) makes oracle/scoring.py::asnorm_stats' statement on them (slice,
    population mean / std) without its matrix product and sort per top: tests/test_scoring_routes_host.py holds the two bit-equal"""

    def __init__(self, E, C):
        S = E.astype(np.float64) @ C.astype(np.float64).T
        self.sorted = -np.sort(-S, axis=1)
        self.smax = float(np.abs(S).max())
        self.K = C.shape[0]

    def stats(self, top):
        S = self.sorted[:, :resolve_top(self.K, top)]
        return S.mean(axis=1), S.std(axis=1)


def summation_bar(K, top, smax):
    """top > 256: top / 64 fp32 terms per lane, then a 6-step butterfly"""
    top = resolve_top(K, top)
    return 4.0 * (top / 64.0 + 6.0) * 2.0 ** -24 * smax if top > FAST_MAX_TOP else 0.0


MU_BAR, SD_REL_BAR, SD_TOP1_BAR = 1e-6, 1e-4, 1e-6    # tests/test_gpu_scoring.py::test_asnorm_stats_vs_oracle
INT_MU_REL, INT_SD_REL = 6e-8, 1e-6


def _worst(err, bar):
    """max err / bar; a bar of zero (an integer mean of exactly 0, the sd of one score) admits an error of zero only"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def stat_errors(data, K, top, mu, sd, rmu, rsd, smax):
    """(mu error / its bar, sd error / its bar), each the worst row: <= 1 passes.  Bars as in the module docstring."""
    extra = summation_bar(K, top, smax)
    mu, sd = np.asarray(mu, np.float64), np.asarray(sd, np.float64)
    if data == "int":
        mu_bar = np.maximum(INT_MU_REL * np.abs(rmu), extra)
        sd_bar = np.maximum(INT_SD_REL * rsd, extra)
    else:
        mu_bar = np.full_like(rmu, max(MU_BAR, extra))
        # 1e-4 of the smallest sd among the rows that have one; a row whose scores are all equal (a zero embedding) and every row at
        # top = 1 have sd = 0 and are held to the top = 1 bar, absolute
        flat = rsd <= 1e-6
        floor = SD_REL_BAR * float(rsd[~flat].min()) if (~flat).any() else SD_TOP1_BAR
        sd_bar = np.maximum(np.where(flat, SD_TOP1_BAR, floor), extra)
    return _worst(np.abs(mu - rmu), mu_bar), _worst(np.abs(sd - rsd), sd_bar)


# ---- d. score_matrix by route ------------------------------------------------------------------------------------------------------------
TILED_WIDTHS, UNALIGNED_WIDTHS = (64, 320, 512), (192, 256)
SIZES = ((1, 5), (129, 64), (70, 130), (260, 33))
# Inside the tiled route the GEMM runs the split form only where gemm_pw takes the shape (api_scoring.hip::score_gemm,
# gemm_pw.hip::gemm_pw_supported: 16-byte aligned operands and output, output rows of Nb % 4 == 0 floats), the fp32 MFMA otherwise: of
# SIZES only 129 x 64.  RAGGED_SPLIT_SIZE adds a second split shape, no whole tile in either direction.
RAGGED_SPLIT_SIZE = (70, 132)
ALL_SIZES = SIZES + (RAGGED_SPLIT_SIZE,)


def split_form_taken(Na, Nb, aligned=True):
    """api_scoring.hip::score_gemm on the tiled route, host or aligned device operands, out (Na, Nb) contiguous"""
    return aligned and Nb % 4 == 0


MAGS = (1.0, 1e3, 3e4, 0.1, 1e-2, 1e-3)
F32_EXTRA_MAGS = (3e5, 1e-6)
TILED_BAR, H3W_BAR = 1e-6, 2e-7       # tests/test_gpu_scoring.py: the tiled bar and the bar of the half-plane test
# The exact fp32 MFMA does not meet the half-plane bar at every magnitude: its worst figure against float64 over the whole table
# (five widths, four sizes, 64 magnitude pairs) is 2.75e-7 of |a||b| on the MI355X, whatever the magnitude; the bar is twice that.
F32MFMA_WORST = 2.75e-7
F32MFMA_BAR = 2 * F32MFMA_WORST
REFUSED_WIDTH = 100
# Proof that the split form ran: with both operands at a row norm of 1e-3 it is 1e-4 of |a||b| from float64 (EMULATED; a factor of two
# either way), the fp32 MFMA within F32MFMA_BAR.  Twenty times that bar lies between the two with room on both sides.
SPLIT_PROOF_NORM, SPLIT_PROOF_ERR = 1e-3, 20 * F32MFMA_BAR
# The served range of the tiled split GEMM, as include/svhip.h and INTEGRATION.md state it: rows of BOTH operands with an L2 norm in
# [lo, hi].  Below lo the lo half of a component goes subnormal (quantum 2^-24) and the error grows as 1 / norm; hi keeps every component
# of a row under the largest half, 65504.  From the device table in MEASURED["tiled"]: the first magnitude that leaves the 1e-6 bar is
# 0.1, with both operands there (1.05e-6 at D = 320); one operand at 0.1 against a row inside the range stays under it (8.4e-7).
TILED_NORM_RANGE = (1.0, 3.0e4)


def in_tiled_range(sa, sb):
    lo, hi = TILED_NORM_RANGE
    return lo <= sa <= hi and lo <= sb <= hi


def matrix_inputs(Na, Nb, D, sa, sb):
    """A (Na, D) of row norm sa, B (Nb, D) of row norm sb, float32 (the norms after the cast are within 1e-7 of sa, sb)"""
    rng = np.random.Generator(np.random.PCG64(Na * 7 + Nb + D))
    return (unit_rows(rng, Na, D) * np.float32(sa)).astype(np.float32), (unit_rows(rng, Nb, D) * np.float32(sb)).astype(np.float32)


def matrix_error(got, A, B):
    """max |got - A B^T| / (|a||b|) against the float64 product"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    scale = np.outer(np.linalg.norm(A64, axis=1), np.linalg.norm(B64, axis=1))
    return float((np.abs(np.asarray(got, np.float64) - A64 @ B64.T) / scale).max())


def half_split_product(A, B):
    """CPU emulation of the tiled route's arithmetic: hi = half(x), lo = half(x - hi), hi.hi + hi.lo + lo.hi, float64 sums"""
    def split(x):
        hi = x.astype(np.float16).astype(np.float32)
        lo = (x - hi).astype(np.float16)
        return hi.astype(np.float64), lo.astype(np.float64)
    ah, al = split(A)
    bh, bl = split(B)
    return ah @ bh.T + ah @ bl.T + al @ bh.T


# error / (|a||b|) of the emulation at row norms 1 .. 1e-4, both operands at the same norm (the table of the issue this module answers);
# the host test holds the emulation to within a factor of two of these at D = 64, 320 and 512
EMULATED = {1.0: 1.0e-7, 0.1: 1.0e-6, 1e-2: 9e-6, 1e-3: 1e-4, 1e-4: 1e-3}

# ---- what the MI355X gave (filled from the GPU test's printed figures) -------------------------------------------------------------------
MEASURED = {
    # asnorm_stats, worst case per (data, form, path): (|mu - ref|, that over its bar, |sd - ref|, that over its bar)
    "stats": {
        ("unit", "reg8", "fast"): (8.76e-08, 0.09, 7.52e-09, 0.00), ("unit", "reg8", "exact"): (1.69e-08, 0.01, 1.57e-08, 0.00),
        ("unit", "reg24", "fast"): (1.22e-07, 0.12, 8.54e-09, 0.00), ("unit", "reg24", "exact"): (3.64e-08, 0.03, 1.11e-08, 0.00),
        ("unit", "lds", "fast"): (1.27e-07, 0.13, 9.95e-09, 0.01), ("unit", "lds", "exact"): (5.58e-08, 0.04, 1.47e-08, 0.01),
        ("unit", "global", "fast"): (1.63e-07, 0.16, 6.86e-09, 0.01), ("unit", "global", "exact"): (3.37e-08, 0.03, 1.13e-08, 0.01),
        ("int", "reg8", "fast"): (7.63e-07, 0.43, 9.15e-07, 0.11), ("int", "reg8", "exact"): (8.81e-07, 0.00, 3.20e-06, 0.00),
        ("int", "reg24", "fast"): (1.53e-06, 0.71, 5.09e-07, 0.09), ("int", "reg24", "exact"): (1.90e-06, 0.01, 8.14e-06, 0.00),
        ("int", "lds", "fast"): (1.83e-06, 0.89, 5.33e-07, 0.10), ("int", "lds", "exact"): (1.86e-06, 0.01, 1.46e-05, 0.00),
    },
    "stats_int_global": {"fast": (1.83e-06, 0.77, 2.92e-07, 0.06), "exact": (1.77e-06, 0.01, 3.10e-07, 0.00)},      # K = 37 892
    # the second split shape, 70 x 132, at norms (1, 1) and (1e-3, 1e-3) per width; and the proof figures of the non-finite test
    "tiled_70x132": {64: (1.07e-07, 1.00e-04), 320: (1.12e-07, 8.69e-05), 512: (1.36e-07, 9.71e-05)},
    "split_proof_at_1e-3": {"split 129 x 64": 9.43e-05, "split 70 x 132": 8.69e-05, "tiled_fp32 70 x 130": 1.58e-07,
                            "unaligned 70 x 130": 1.29e-07, "f32mfma 70 x 130": 1.58e-07},
    "odd_K7000": dict(mu=7.43e-08, sd_rel=2.97e-06, zero_row_sd=0.0, fallback_rows=3),
    "two_slabs": dict(mu=2.40e-08, sd_rel=1.27e-07, free_before_MiB=293750, free_after_MiB=293734),
    "census": (("asnorm_topk_global", "asnorm_topk_lds", "asnorm_topk_reg24", "asnorm_topk_reg8"), (1, 2, 3, 4)),
    # tiled route, error / (|a||b|), worst over D = 64, 320, 512 and the four sizes; rows |a|, columns |b| in the order of MAGS.  Of the
    # four sizes only 129 x 64 runs the split form (the others fall to the fp32 MFMA inside the same route: 1e-7 at every magnitude).
    "tiled": {
        1.0: (1.7e-07, 1.7e-07, 1.5e-07, 7.2e-07, 8.2e-06, 6.5e-05),
        1e3: (1.6e-07, 1.7e-07, 1.6e-07, 7.2e-07, 8.2e-06, 6.5e-05),
        3e4: (1.6e-07, 1.6e-07, 1.7e-07, 7.1e-07, 8.2e-06, 6.5e-05),
        0.1: (8.0e-07, 8.3e-07, 8.4e-07, 1.05e-06, 8.0e-06, 6.5e-05),
        1e-2: (6.8e-06, 6.8e-06, 6.8e-06, 6.8e-06, 1.1e-05, 6.6e-05),
        1e-3: (7.1e-05, 7.1e-05, 7.1e-05, 7.1e-05, 7.1e-05, 9.9e-05),
    },
    # D = 192 / 256 with unaligned operands: split_words runs, the GEMM itself is the fp32 MFMA (the split form wants 16-byte rows)
    "tiled_unaligned": {192: 2.2e-07, 256: 1.9e-07},
    "f32mfma": {64: 2.75e-07, 320: 2.08e-07, 512: 1.88e-07, 192: 2.20e-07, 256: 2.59e-07},
    "f32mfma_asnorm_stats": (0.01, 0.00), "f32mfma_score_topk": 1.68e-07,
    "unaligned_asnorm_stats": (0.03, 0.00),
    "pairs": {(192, 4): (1.19e-07, 5.98e-08), (320, 4): (1.19e-07, 9.01e-08), (512, 4): (1.19e-07, 3.56e-08), (1, 0): (0.0, 9.18e-08),
              (30, 0): (1.19e-07, 9.02e-08)},
}
