"""Edge cases, references and reference mutants of the quantizer kernels of csrc/vt_vq.hip (vt_vq_forward, vt_vq_backward, vt_vq_gather,
vt_vq_prep_codebook).  numpy, torch on the CPU and the C oracle (oracle/vq_oracle.c): no GPU and no built library.  The pattern is that
of tests/attention_cases.py and tests/gated_cases.py.

FORWARD.  A case is (name, N, K, d, mode L | D, l2_normalized, ldz, ldp, specials) with inputs drawn from oracle/inputs.py seeds.  Its
REFERENCE is the oracle, which claims the kernel's fp32 order, so every comparison on the asserted tokens is array_equal.  The oracle
costs seconds on the large shapes, so those carry a fixed TOKEN SUBSET (`token_subset`): tokens are independent, the oracle on z[sel]
is exact.  Specials are planted into the inputs:
    ties         (kind, i, j, token): W[j] = W[i] (i < j) and z[token] = W[i]; both copies score the same bits, the answer is i.  kind
                 says where the copies sit for the planner as committed: 'half' (the two lane halves of one 32-code tile), 'tile' (two
                 tiles of one chunk, same lane half), 'chunk' (two chunks of one split), 'split' (two splits)
    hits         (code, token): z[token] = W[code], so that a given tile / chunk / split holds a known winner
    zero_tokens  a zero row normalises to 0 through the 1e-12 clamp: mode D ties every code at 0 (answer 0), mode L ties the codes whose
                 fl(|e|^2) is smallest
    zero_codes   E row 0, wnorm 1e-12
A MUTANT is the oracle on transformed inputs (so it stays bit-exact without a second fma chain): the index vector a kernel with one
thing miscounted would give.  It is CAUGHT by a case when that vector differs from the reference's on the case's asserted tokens
(tests/test_vq_cases_cpu.py requires every mutant caught and every case to catch what it was built for).  On a subset case the mutants
are evaluated on the special tokens only: those are what the large shapes add.

`split_plan` and `cb_plan` restate vq_split_plan and cb_slabs / slab_len of csrc/vt_vq.hip.  They are used only to assert that a case
still reaches what it claims (`claims`, the kinds of its ties): after a retuned planner the CPU test names the case that lost its purpose.

TOKEN BACKWARD.  The reference is a float64 torch restatement of the reference module's forward (F.normalize, q = E[idx], the three
losses, rz = z + (q - z).detach()) differentiated by autograd; the bar per element is analytic from the float64 operands (`bwd_reference`);
`bwd_replay` is the kernel's formula in float32, which the CPU test requires inside the bar.  No bar comes from a kernel's output."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import inputs as gen
from oracle import vq_c

CHUNK, TILE, WG = 128, 32, 256          # codes per LDS chunk, codes / tokens per MFMA tile, tokens per workgroup
POISON16, POISON32, POISON64 = 0x4B4B, 0x4B4B4B4B, 0x4B4B4B4B4B4B4B4B
PF = float(np.array([POISON32], dtype=np.uint32).view(np.float32)[0])     # finite (13323083.0): input padding holds it too
TAIL = 3                                 # rows behind every output: it is a view of a larger allocation
INV_TAU = float(np.float32(1.0 / 0.03))
BETA, CBW = float(np.float32(0.4)), float(np.float32(0.6))      # the fp32 values the C ABI receives
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ planner restatement
def split_plan(N, K):
    Kp = (K + CHUNK - 1) // CHUNK * CHUNK
    tblocks, nchunks = (N + WG - 1) // WG, Kp // CHUNK
    want = min(max(768 // tblocks, 1), nchunks)
    cps = (nchunks + want - 1) // want
    nsplit = (nchunks + cps - 1) // cps
    return {"Kp": Kp, "tblocks": tblocks, "nchunks": nchunks, "cps": cps, "nsplit": nsplit, "last": nchunks - (nsplit - 1) * cps}


def cb_plan(N):
    ns = min(32, max(1, (N + 511) // 512))
    slab_len = ((N + ns - 1) // ns + 63) // 64 * 64
    lens = [max(0, min(N, (s + 1) * slab_len) - s * slab_len) for s in range(ns)]
    return {"ns": ns, "slab_len": slab_len, "empty": sum(1 for v in lens if v == 0), "last_len": [v for v in lens if v][-1],
            "partial_chunk": sum(1 for v in lens if v % 64)}


def workspace_floats(N, K, d):
    """vt_vq_workspace_bytes / 4, and the part of it the forward writes"""
    p = split_plan(N, K)
    fwd = d * p["Kp"] + p["Kp"] + N + 2 * p["nsplit"] * N + p["tblocks"]
    return max(fwd + 64, cb_plan(N)["ns"] * K * d), fwd


def tie_kind(i, j, N, K):
    p = split_plan(N, K)
    span = p["cps"] * CHUNK
    if i // span != j // span:
        return "split"
    if i // CHUNK != j // CHUNK:
        return "chunk"
    if i // TILE != j // TILE:
        return "tile" if (i % 8 < 4) == (j % 8 < 4) else "tile+half"
    return "half" if i % 8 < 4 <= j % 8 else "lane"


# ------------------------------------------------------------------------------------------------ forward cases
class Case:
    def __init__(self, name, N, K, d, mode, l2n=1, strided=True, ties=(), hits=(), zero_tokens=(), zero_codes=(), stride=0, claims=None,
                 must_catch=(), seed=0):
        self.name, self.N, self.K, self.d, self.mode, self.l2n = name, N, K, d, mode, l2n
        self.ldz, self.ldp = (d + 8 if strided else d), 64
        self.ties, self.hits, self.zero_tokens, self.zero_codes = tuple(ties), tuple(hits), tuple(zero_tokens), tuple(zero_codes)
        self.stride, self.claims, self.must_catch, self.seed = stride, dict(claims or {}), tuple(must_catch), seed

    @property
    def subset(self):
        return self.stride > 0

    @property
    def special_tokens(self):
        return sorted({t for *_, t in self.ties} | {t for _, t in self.hits} | set(self.zero_tokens))


def _build_cases():
    cs = []
    # every d instantiation x both modes, ragged everything: K = 300 pads to 384, the last 32-code tile holds 12 codes, N = 289 leaves a
    # 33-token workgroup.  cps = 1, so two chunks are two splits.
    ties300 = (("half", 33, 38, 3), ("tile", 5, 70, 40), ("split", 7, 135, 260), ("split", 200, 299, 288))
    for d in (8, 16, 24, 32):
        for mode in "LD":
            cs.append(Case(f"ragged_d{d}_{mode}", 289, 300, d, mode, ties=ties300, hits=((297, 287),),
                           zero_tokens=(100,) if d in (16, 24) else (), zero_codes=(150,) if d in (8, 32) else (),
                           claims={"cps": 1, "nsplit": 3, "Kp": 384, "tblocks": 2},
                           must_catch=("ties_high", "drop_last_tile", "drop_last_chunk", "tail_clamped", "ldz_as_d", "upper_half_ignored")))
    # tiny extremes
    for (N, K), d in zip(((1, 1), (1, 5), (31, 127), (257, 129)), (8, 16, 24, 32)):
        for mode in "LD":
            cs.append(Case(f"tiny_N{N}_K{K}_d{d}_{mode}", N, K, d, mode, ties=(("split", 2, 128, 256),) if K == 129 else (),
                           claims={"cps": 1}, must_catch=("ties_high", "tail_clamped") if K == 129 else ()))
    # unmasked-padding detector: five unit codes, most tokens farther than 1 from all of them (mode L) / with only negative cosines (mode D)
    for mode in "LD":
        cs.append(Case(f"pad5_d24_{mode}", 64, 5, 24, mode, claims={"Kp": 128, "nsplit": 1}, must_catch=("pad_unmasked",)))
    # deep chunk loop: cps = 3 rewrites LDS buffer 0, the last split holds one chunk
    K = 15437
    deep = dict(ties=(("half", 1025, 1030, 5), ("tile", 390, 455, 300), ("chunk", 10, 138, 700), ("chunk", 20, 276, 1300), ("chunk", 7700, 7950, 2000),
                      ("split", 50, K - 3, 3072)),
                hits=((K - 1, 2900), (128 + 77, 1000), (256 + 99, 1001), (40 * 384 - 1, 1002)), stride=13,
                claims={"tblocks": 13, "nchunks": 121, "cps": 3, "nsplit": 41, "last": 1}, must_catch=("ties_high", "drop_last_split", "drop_last_tile"))
    cs.append(Case("deep_d8_L", 3073, K, 8, "L", **deep))
    cs.append(Case("deep_d32_D", 3073, K, 32, "D", **deep))
    cs.append(Case("deep_d24_L", 3073, K, 24, "L", **deep))
    # cps = 4, many token blocks
    K = 6145
    cs.append(Case("cps4_d16_L", 12288, K, 16, "L", stride=37,
                   ties=(("half", 513, 519, 9), ("chunk", 30, 30 + 3 * CHUNK, 4100), ("chunk", 2100, 2100 + 2 * CHUNK, 8000), ("split", 60, 5000, 12287)),
                   hits=((K - 1, 12000), (3 * CHUNK + 5, 6000), (6143, 6001)),
                   claims={"tblocks": 48, "nchunks": 49, "cps": 4, "nsplit": 13, "last": 1}, must_catch=("ties_high", "drop_last_split")))
    # un-normalised (mode L only; inputs scaled by 3)
    for d in (8, 24):
        cs.append(Case(f"raw_d{d}_L", 289, 300, d, "L", l2n=0, ties=ties300, hits=((297, 287),), zero_codes=(150,) if d == 8 else (),
                       claims={"cps": 1, "nsplit": 3}, must_catch=("ties_high", "ldz_as_d")))
    for n, c in enumerate(cs):
        c.seed = 7100 + 10 * n
    return collections.OrderedDict((c.name, c) for c in cs)


CASES = _build_cases()


def names(subset=None):
    return [n for n, c in CASES.items() if subset is None or c.subset == subset]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(W [K, d], backing [N, ldz]): the tokens are columns [0, d) of backing, the rest of it holds poison"""
    c = CASES[name]
    scale = np.float32(1.0 if c.l2n else 3.0)
    W = gen.kaiming_uniform_codebook(c.K, c.d, c.seed) * scale
    z = gen.normal((c.N, c.d), c.seed + 1000) * scale
    for k in c.zero_codes:
        W[k] = 0.0
    for _, i, j, t in c.ties:
        W[j] = W[i]
        z[t] = W[i]
    for k, t in c.hits:
        z[t] = W[k]
    for t in c.zero_tokens:
        z[t] = 0.0
    backing = np.full((c.N, c.ldz), PF, dtype=np.float32)
    backing[:, :c.d] = z
    W.setflags(write=False)
    backing.setflags(write=False)
    return W, backing


def token_subset(c):
    """the asserted tokens: all of them, or on a subset case the first and last token of every workgroup and of the 32-token tiles at its
    two ends, every token of a partial last workgroup, every special token and a fixed stride through the rest"""
    if not c.subset:
        return np.arange(c.N)
    s = set(c.special_tokens) | set(range(0, c.N, c.stride))
    for w0 in range(0, c.N, WG):
        hi = min(c.N, w0 + WG)
        s.update(range(w0, hi) if hi - w0 < WG else (w0, w0 + TILE - 1, hi - TILE, hi - 1))
    return np.array(sorted(s))


Ref = collections.namedtuple("Ref", "sel zn znorm E wnorm idx rz q mse")


def _normalised(c, z_in, W):
    if c.l2n:
        zn, znorm = vq_c.normalize_rows(z_in)
        E, wnorm = vq_c.normalize_rows(W)
        return zn, znorm, E, wnorm
    return (np.ascontiguousarray(z_in, dtype=np.float32), np.ones(z_in.shape[0], np.float32), np.ascontiguousarray(W, dtype=np.float32),
            np.ones(W.shape[0], np.float32))


@functools.lru_cache(maxsize=None)
def reference(name):
    """zn, znorm, E, wnorm for every row (cheap); idx, rz, q on `sel`; mse (float64) on full-oracle cases, else None"""
    c = CASES[name]
    W, backing = inputs(name)
    zn, znorm, E, wnorm = _normalised(c, backing[:, :c.d], W)
    sel = token_subset(c)
    idx, _ = vq_c.search(zn[sel], E, c.mode, INV_TAU)
    q, rz, tot = vq_c.gather(zn[sel], E, idx)
    return Ref(sel, zn, znorm, E, wnorm, idx, rz, q, None if c.subset else tot / (c.N * c.d))


# ------------------------------------------------------------------------------------------------ mutants
def _tokens(c, r):
    """positions in r.sel a mutant is evaluated on"""
    if not c.subset:
        return np.arange(len(r.sel))
    return np.searchsorted(r.sel, np.array(c.special_tokens))


def _search(c, z, E):
    return vq_c.search(z, E, c.mode, INV_TAU)[0]


def _m_ties_high(c, r, pos):
    return c.K - 1 - _search(c, r.zn[r.sel[pos]], r.E[::-1])


def _drop(c, r, pos, keep):
    if keep <= 0 or keep >= c.K:
        return None
    return _search(c, r.zn[r.sel[pos]], r.E[:keep])


def _m_drop_tile(c, r, pos):
    return _drop(c, r, pos, (c.K - 1) // TILE * TILE)


def _m_drop_chunk(c, r, pos):
    return _drop(c, r, pos, (c.K - 1) // CHUNK * CHUNK)


def _m_drop_split(c, r, pos):
    p = split_plan(c.N, c.K)
    return _drop(c, r, pos, (p["nsplit"] - 1) * p["cps"] * CHUNK)


def _m_pad(c, r, pos):
    Kp = split_plan(c.N, c.K)["Kp"]
    if Kp == c.K:
        return None
    return _search(c, r.zn[r.sel[pos]], np.concatenate([r.E, np.zeros((Kp - c.K, c.d), np.float32)]))


def _m_tail(c, r, pos):
    out = r.idx[pos].copy()
    tok = r.sel[pos]
    a, b = np.nonzero(tok == c.N - 1)[0], np.nonzero(tok == c.N - 2)[0]
    if c.N < 2 or not len(a) or not len(b):
        return None
    out[a[0]] = out[b[0]]
    return out


def _m_ldz(c, r, pos):
    if c.ldz == c.d:
        return None
    _, backing = inputs(c.name)
    z = backing.reshape(-1)[:c.N * c.d].reshape(c.N, c.d)[r.sel[pos]]
    return _search(c, vq_c.normalize_rows(z)[0] if c.l2n else z, r.E)


def _m_half(c, r, pos):
    keep = np.nonzero(np.arange(c.K) % 8 < 4)[0]
    return keep[_search(c, r.zn[r.sel[pos]], r.E[keep])]


MUTANTS = collections.OrderedDict([
    ("ties_high", _m_ties_high),                # the highest index wins a tie: the oracle on the row-reversed codebook, indices mapped back
    ("split_merge_non_strict", _m_ties_high),   # vq_finalize_kernel taking the later split on equal scores: the same vector on 'split' ties
    ("drop_last_tile", _m_drop_tile),           # the last 32-code tile / 128-code chunk / split never searched
    ("drop_last_chunk", _m_drop_chunk),
    ("drop_last_split", _m_drop_split),
    ("pad_unmasked", _m_pad),                   # `code < K` missing: zero codes up to Kp take part, un-normalised
    ("tail_clamped", _m_tail),                  # the token tail clamped one short: token N-1 answers as token N-2
    ("ldz_as_d", _m_ldz),                       # the row stride of z_in taken as d
    ("upper_half_ignored", _m_half),            # the merge of the two lane halves dropped: only the codes with code % 8 < 4
])


def mutant_idx(name, mutant):
    """(positions in sel, index vector of the mutant there) or None where the mutant is provably the reference"""
    c, r = CASES[name], reference(name)
    pos = _tokens(c, r)
    if mutant == "split_merge_non_strict" and not any(k == "split" for k, *_ in c.ties):
        return None
    if not len(pos):
        return None
    got = MUTANTS[mutant](c, r, pos)
    return None if got is None else (pos, got)


def caught(name, mutant):
    m = mutant_idx(name, mutant)
    return m is not None and not np.array_equal(m[1], reference(name).idx[m[0]])


# ------------------------------------------------------------------------------------------------ all-token score check
def score_gap_and_bound(zn, E, idx, mode, inv_tau=INV_TAU, block=2048):
    """For every token: how far the chosen code's float64 score is from the row's best, and the bound on that for an honest fp32 search:
    an fp32 score differs from the float64 one by at most b(code) = (d + 2) 2^-24 (|z|^2 + |e|^2 + 2 sum|z_k e_k|) in mode L and
    (d + 2) 2^-24 sum|z_k e_k| inv_tau in mode D, so chosen and best are within b(chosen) + b(best).  torch tensors (any device),
    float32 operands as the kernel wrote them; returns float64 (gap, bound)."""
    z, e = zn.double(), E.double()
    d = z.shape[1]
    gaps, bounds = [], []
    ee = (e * e).sum(1)
    for a in range(0, z.shape[0], block):
        zb, ib = z[a:a + block], idx[a:a + block]
        dot, adot = zb @ e.T, zb.abs() @ e.abs().T
        if mode == "L":
            sc = (zb * zb).sum(1, keepdim=True) + ee[None] - 2.0 * dot
            bnd = (d + 2) * U * ((zb * zb).sum(1, keepdim=True) + ee[None] + 2.0 * adot)
            best = sc.argmin(1, keepdim=True)
            gap = sc.gather(1, ib[:, None]) - sc.gather(1, best)
        else:
            sc = dot * inv_tau
            bnd = (d + 2) * U * adot * inv_tau
            best = sc.argmax(1, keepdim=True)
            gap = sc.gather(1, best) - sc.gather(1, ib[:, None])
        gaps.append(gap[:, 0])
        bounds.append((bnd.gather(1, ib[:, None]) + bnd.gather(1, best))[:, 0])
    return torch.cat(gaps), torch.cat(bounds)


# ------------------------------------------------------------------------------------------------ token backward
GSCAL = tuple(float(np.float32(v)) for v in (0.7, 0.3, 0.45))   # d loss_q, d loss_commit, d loss_codebook: non-zero, distinct, fp32 values
BWD_K = 77
BWD_VARIANTS = ("dz_in", "dz_pad", "both", "no_g_rz")
BWD_D, BWD_N = (8, 16, 24, 32), (1, 255, 257, 700)


def bwd_cases():
    """(N, d, l2n, variant): every d meets every variant, with both l2_normalized values"""
    return [(N, d, l2n, BWD_VARIANTS[(a + b) % 4]) for l2n in (1, 0) for a, d in enumerate(BWD_D) for b, N in enumerate(BWD_N)]


@functools.lru_cache(maxsize=None)
def bwd_inputs(N, K, d, l2n, collapse=0):
    """W, z (no zero rows), g backing [N, d + 8] whose columns >= d hold poison.  collapse = n: the first n tokens sit next to code 7."""
    seed = 9000 + 7 * N + 131 * d + 3 * K + l2n
    scale = np.float32(1.0 if l2n else 3.0)
    W = gen.kaiming_uniform_codebook(K, d, seed) * scale
    z = gen.normal((N, d), seed + 1000) * scale
    if collapse:
        z[:collapse] = W[min(7, K - 1)] + np.float32(0.01) * z[:collapse]
    g = np.full((N, d + 8), PF, dtype=np.float32)
    g[:, :d] = gen.normal((N, d), seed + 2000)
    for a in (W, z, g):
        a.setflags(write=False)
    return W, z, g


def bwd_reference(z_in, W, idx, g, gscal, l2n, beta=BETA, cbw=CBW):
    """float64: (dz_in, dW, bar of dz_in).  g may be None.  The bar: with s_c = (|gscal0| beta + |gscal1|) 2 / (N d) (magnitudes: the
    two terms may cancel) and A_j = |g_j| + s_c (|z_j| + |e_j|) the magnitude of what is
    summed into dz_j, an fp32 evaluation of (dz - z (z.dz)) / |z_in| is off by at most (2d + 16) 2^-24 (A_j + |z_j| sum_k |z_k| A_k) / |z_in|:
    d roundings in each of the two d-long sums (|z_in|^2, whose error scales every z_k, and z.dz), and a fixed handful for s_c, the
    difference, the product, the subtraction and the division.  Without normalisation only the handful is left: 8 * 2^-24 A_j."""
    z_in = torch.from_numpy(np.array(z_in)).double().requires_grad_(True)
    W = torch.from_numpy(np.array(W)).double().requires_grad_(True)
    idx = torch.from_numpy(np.array(idx))
    z = F.normalize(z_in, dim=-1) if l2n else z_in
    E = F.normalize(W, dim=-1) if l2n else W
    q = E[idx]
    commit = ((q.detach() - z) ** 2).mean()
    codebook = ((q - z.detach()) ** 2).mean()
    loss_q = beta * commit + cbw * codebook
    rz = z + (q - z).detach()
    total = gscal[0] * loss_q + gscal[1] * commit + gscal[2] * codebook
    gd = None
    if g is not None:
        gd = torch.from_numpy(np.array(g)).double()
        total = total + (gd * rz).sum()
    dz, dW = torch.autograd.grad(total, (z_in, W))
    N, d = z.shape
    with torch.no_grad():
        s_c = (abs(gscal[0]) * beta + abs(gscal[1])) * 2.0 / (N * d)
        A = s_c * (z.abs() + q.abs()) + (gd.abs() if gd is not None else 0.0)
        if l2n:
            bar = (2 * d + 16) * U * (A + z.abs() * (z.abs() * A).sum(1, keepdim=True)) / z_in.norm(dim=1, keepdim=True)
        else:
            bar = 8 * U * A
    return dz, dW, bar


def bwd_bar_bf16(want, bar):
    """the bar of the bf16 copy: the fp32 bar, plus half a bf16 step (at most 2^-8 of the value) of anything within it"""
    return bar + 2.0 ** -8 * (want.abs() + bar)


def bwd_replay(zn, znorm, E, idx, g, gscal, l2n, beta=BETA, cbw=CBW):
    """the formula of vq_bwd_tokens_kernel in float32 numpy (sequential sums): what an honest fp32 kernel may give"""
    f = np.float32
    N, d = zn.shape
    s_c = f(f(f(f(gscal[0]) * f(beta)) + f(gscal[1])) * f(2.0)) / f(f(N) * f(d))
    e = E[idx]
    dz = (g.astype(f) if g is not None else np.zeros_like(zn)) + s_c * (zn - e)
    if not l2n:
        return dz.astype(f)
    dot = np.zeros(N, dtype=f)
    for j in range(d):
        dot = dot + zn[:, j] * dz[:, j]
    inv = f(1.0) / znorm
    return ((dz - zn * dot[:, None]) * inv[:, None]).astype(f)


# ------------------------------------------------------------------------------------------------ codebook gradient
def cbgrad_cases():
    """(N, K, d, l2n, collapse): d in {8, 32}, K off every tile size, N at 1 / below a chunk / two slabs / eight slabs with one token in
    the last / the 32-slab cap with three empty slabs; l2_normalized = 0 on a part; collapse = the first slab sits on one code"""
    out = []
    for d in (8, 32):
        for K in (5, 77, 300):
            for N in (1, 63, 513, 3585):
                l2n = 0 if (K == 77 or (K == 300 and N == 513)) and d == 8 or (K == 5 and d == 32) else 1
                out.append((N, K, d, l2n, 512 if N == 3585 and K != 5 else 0))
    out.append((16385, 77, 8, 1, 0))
    out.append((16385, 77, 8, 0, 576))
    return out


def s_b_fp32(gscal, N, d, cbw=CBW):
    f = np.float32
    return f(f(f(f(gscal[0]) * f(cbw)) + f(gscal[2])) * f(2.0)) / f(f(N) * f(d))
