"""Training every missing-modality pattern of an MMIMDb batch in one step, the parts that need no device.

The derivation the step rests on, in fp64 on the CPU oracle: the encoders' input BatchNorm1d statistics of the replicated
P·B-row batch from the B real rows, the one row every all-zero input normalises to, the encoders over B + 1 rows, the fold
of the fusion-input gradient onto those rows and the BatchNorm dgamma / dbeta from them reproduce ``orc.train_step`` on
the explicitly replicated and masked batch (logits, loss, every parameter gradient, the running statistics).

The three entry points ``tspm_bn1d_fwd_rep``, ``tspm_bn1d_fwd_rep_pair``, ``tspm_gmu_pattern_bwd`` (export, header and
ctypes agree; every refusal returns before any launch, so it runs without a device; the workspace query) and the
constructor checks of ``FusedMMIMDbPatternStep`` that come before anything touches a device."""
import copy
import ctypes
import os
import re

import pytest
import torch

from oracle import mmimdb_ref as orc
from parity import rel_l2
from tspm_amd import _lib as L
from tspm_amd import mmimdb as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "tspm.h")
OK, INVALID, WORKSPACE = 0, 1, 3
FAKE = 0x10000  # a non-NULL value: a refused call never dereferences (or launches with) it
_ids = lambda rs: [",".join(f"{k}={v}" for k, v in r.items())[:40] for r in rs]  # noqa: E731


# ------------------------------------------------------------------------------------------------
# the derivation, in fp64
# ------------------------------------------------------------------------------------------------
DIMS = dict(image_dim=40, text_dim=12, embed=16, hidden=8, genres=5)
PATTERN_SETS = [("it", "i", "t"), ("t", "it"), ("it",)]
POOLING = {"pooling_type": "attention", "hidden_dim": 8, "dropout": 0.1}


def _oracle64(pooling):
    """A small fp64 oracle model in train mode with non-trivial BatchNorm affine parameters and running statistics.

    eps = 0.1 in every BatchNorm1d, for the conditioning of the two-row cases (B = 1 under two patterns).  Over two rows
    xhat = ±c with c² = var / (var + eps), and the BatchNorm backward g - mean(g) - xhat·mean(g·xhat) comes to
    (1 - c²)·(g1 - g2)/2: at eps = 1e-5 every gradient above a two-row BatchNorm is the 1e-5-sized remnant of a
    cancellation, which fp64 forms to ~1e-11 of its value in the oracle and in any restatement of it alike (measured
    here at the default eps: 1.1e-12 on text_model.net.0.bias, 1.3e-11 on mm_mlp.net.4.layers.0.weight, every case
    of three or more rows at or below 7e-14).  With eps = 0.1 against variances of order 0.1..1 the factor 1 - c² is
    0.1 or more per layer, so 1e-12 measures the derivation in every case, not fp64's cancellation; eps enters the
    statistics formulas under test as it does at 1e-5."""
    m = orc.build_oracle_mmimdb(3, pooling=pooling, **DIMS).double()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.eps = 0.1
                c = mod.num_features
                mod.running_mean.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.3)
                mod.running_var.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
                mod.weight.copy_(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.2)
    return m.train()


def _fuse(m, U, keep_pool):
    """The fusion after its two projections, in train mode, on U = [proj(image) | proj(text)]."""
    f, d = m.fusion_module, U.shape[1] // 2
    a, b = torch.tanh(U[:, :d]), torch.tanh(U[:, d:])
    if m.fusion_type != "pooling":
        g = torch.sigmoid(f.hidden_sigmoid(torch.cat([a, b], dim=1)))
        return g * a + (1 - g) * b
    s = 1.0 / (1.0 - f.dropout)
    a, b = a * (keep_pool[0].to(a.dtype) * s), b * (keep_pool[1].to(b.dtype) * s)
    w = f.attention_layer(torch.cat([a, b], dim=1))
    return w[:, :1] * a + w[:, 1:] * b


def _b_plus_1_step(m, I, T, y, pats, keep1, keep2, keep_pool):
    """The all-pattern step as the HIP path runs it: statistics of the replicated batch from the B real rows, the
    encoders over B + 1 rows, the fusion and the classifier over P·B rows, the gradient folded back onto B + 1 rows and
    the input BatchNorms' dgamma / dbeta formed from them.  Returns (logits, loss, {parameter name: gradient},
    {buffer name: running statistic})."""
    B, P = I.shape[0], len(pats)
    N = P * B
    f = m.fusion_module
    projs = (f.proj_a, f.proj_b) if m.fusion_type == "pooling" else (f.fc_one, f.fc_two)
    grads, running, halves, bn_state = {}, {}, [], []
    for mi, (name, enc, x, proj) in enumerate((("image_model", m.image_model, I, projs[0]),
                                               ("text_model", m.text_model, T, projs[1]))):
        bn, fc = enc.net[0], enc.net[1]
        k = sum(1 for p in pats if M.PATTERNS[p][mi])
        S = x.sum(0)
        mean = k * S / N
        M2 = k * ((x - mean) ** 2).sum(0) + (P - k) * B * mean ** 2
        invstd = 1.0 / torch.sqrt(M2 / N + bn.eps)
        running[f"{name}.net.0.running_mean"] = (1 - bn.momentum) * bn.running_mean + bn.momentum * mean
        running[f"{name}.net.0.running_var"] = (1 - bn.momentum) * bn.running_var + bn.momentum * M2 / (N - 1)
        x1 = torch.cat([x, torch.zeros_like(x[:1])])                     # B + 1 rows: the last is the zero input
        xhat = (x1 - mean) * invstd
        Xn = (xhat * bn.weight + bn.bias).detach().requires_grad_(True)  # row B: what every zero row normalises to
        halves.append(proj(fc(Xn)))                                      # row-wise: one extra row
        bn_state.append((name, bn, xhat.detach(), Xn))
    U = torch.cat(halves, dim=1)                                         # [B + 1, 2d]; U[B] is the zero row's
    d = U.shape[1] // 2
    rows = []
    for p in pats:
        ip, tp = M.PATTERNS[p]
        rows.append(torch.cat([U[:B, :d] if ip else U[B:, :d].expand(B, d), U[:B, d:] if tp else U[B:, d:].expand(B, d)], 1))
    Ux = torch.cat(rows).detach().requires_grad_(True)                   # [P·B, 2d], a leaf: the fold below is explicit
    logits = m.mm_mlp(_fuse(m, Ux, keep_pool), keep1, keep2)
    loss = orc.bce_loss(logits, y.repeat(P, 1))
    for q in m.parameters():
        q.grad = None
    loss.backward()
    # the fold: row b sums the patterns that keep the modality, row B every sample under every pattern that drops it
    dU = torch.zeros_like(U)
    for pi, p in enumerate(pats):
        gp = Ux.grad[pi * B:(pi + 1) * B]
        for half, kept in ((slice(0, d), M.PATTERNS[p][0]), (slice(d, 2 * d), M.PATTERNS[p][1])):
            if kept:
                dU[:B, half] += gp[:, half]
            else:
                dU[B, half] += gp[:, half].sum(0)
    U.backward(dU)                                                       # every Linear backward over the B + 1 rows
    for name, bn, xhat, Xn in bn_state:                                  # the input BNs: only dgamma / dbeta are needed
        grads[f"{name}.net.0.weight"] = (Xn.grad * xhat).sum(0)
        grads[f"{name}.net.0.bias"] = Xn.grad.sum(0)
    for n_, q in m.named_parameters():
        if n_ not in grads:
            grads[n_] = q.grad.detach().clone()
    for n_, b_ in m.named_buffers():
        if ("running" in n_) and n_ not in running:
            running[n_] = b_.detach().clone()                            # the classifier's BNs ran in autograd above
    return logits.detach(), loss.detach(), grads, running


# B = 1 with ("it",) alone is a one-row batch: BatchNorm1d in training mode rejects it, in the oracle and in the step
CASES = [(B, pats) for B in (1, 5) for pats in PATTERN_SETS if B * len(pats) >= 2]


@pytest.mark.parametrize("pooling", [None, POOLING], ids=["gmu", "attention"])
@pytest.mark.parametrize("B,pats", CASES, ids=[f"B{B}-{'+'.join(p)}" for B, p in CASES])
def test_b_plus_1_rows_reproduce_the_replicated_batch(B, pats, pooling):
    P = len(pats)
    I, T, y = orc.synthetic_batch(B, seed=5, image_dim=DIMS["image_dim"], text_dim=DIMS["text_dim"],
                                  genres=DIMS["genres"])
    I, T, y = I.double(), T.double(), y.double()
    g = torch.Generator().manual_seed(B * 10 + P)
    N, h, d = P * B, DIMS["hidden"], DIMS["embed"]
    keep1, keep2 = ((torch.rand(N, h, generator=g) >= 0.5).to(torch.uint8) for _ in range(2))
    keep_pool = None if pooling is None else tuple((torch.rand(N, d, generator=g) >= 0.1).to(torch.uint8)
                                                   for _ in range(2))
    ours_m, ref_m = _oracle64(pooling), _oracle64(pooling)
    logits, loss, grads, running = _b_plus_1_step(ours_m, I, T, y, pats, keep1, keep2, keep_pool)
    Irep = torch.cat([I * M.PATTERNS[p][0] for p in pats])
    Trep = torch.cat([T * M.PATTERNS[p][1] for p in pats])
    r = orc.train_step(ref_m, None, Irep, Trep, y.repeat(P, 1), keep1, keep2, None, keep_pool)
    worst = max(rel_l2(logits, r["logits"]), rel_l2(loss, r["loss"]))
    assert worst <= 1e-12, ("logits / loss", worst)
    for name, q in ref_m.named_parameters():
        e = rel_l2(grads[name], q.grad)
        worst = max(worst, e)
        assert e <= 1e-12, (name, e)
    n_stats = 0
    for name, b_ in ref_m.named_buffers():
        if "running" in name:
            e = rel_l2(running[name], b_)
            worst = max(worst, e)
            n_stats += 1
            assert e <= 1e-12, (name, e)
    assert n_stats == 10  # five BatchNorm1d layers
    print(f"B={B} {'+'.join(pats)} {'gmu' if pooling is None else 'attention'}: worst rel-L2 {worst:.2e}")


# ------------------------------------------------------------------------------------------------
# header, export, binding
# ------------------------------------------------------------------------------------------------
def test_header_export_and_binding_agree():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int tspm_bn1d_fwd_rep(int32_t m, int32_t c, const float* x, const float* gamma, const float* beta, "
            "float* running_mean, float* running_var, float momentum, float eps, float* save_mean, float* save_invstd, "
            "float* y, int32_t reps, int32_t zero_rows_per_row, tspm_stream_t stream);") in src
    assert "int tspm_bn1d_fwd_rep_pair(int32_t m, int32_t c0, const float* x0," in src
    assert ("int tspm_gmu_pattern_bwd(int32_t batch, int32_t npat, const int32_t* keep, int32_t d, const float* dz, "
            "int32_t lddz, const float* h, int32_t ldh, const float* gate, const float* wz, float* du, int32_t lddu, "
            "float* ds, void* workspace, size_t workspace_bytes, tspm_stream_t stream);") in src
    assert "size_t tspm_gmu_pattern_bwd_workspace(int32_t batch, int32_t d);" in src
    assert "#define TSPM_ABI_VERSION 23 " in src and L.ABI_VERSION == 23 and L.lib().tspm_abi_version() == 23
    so = ctypes.CDLL(L.LIB_PATH)
    for name in ("tspm_bn1d_fwd_rep", "tspm_bn1d_fwd_rep_pair", "tspm_gmu_pattern_bwd",
                 "tspm_gmu_pattern_bwd_workspace"):
        assert name in L.EXPORTED and hasattr(so, name)
    assert M.DEFAULT_TRAIN_PATTERN_FUSION in ("kernel", "launches")


# ------------------------------------------------------------------------------------------------
# tspm_bn1d_fwd_rep / _pair
# ------------------------------------------------------------------------------------------------
BN_KEYS = ("c", "x", "gamma", "beta", "running_mean", "running_var", "momentum", "eps", "save_mean", "save_invstd", "y",
           "reps", "zero_rows_per_row")
BN_GOOD = dict(m=5, c=36, x=FAKE, gamma=FAKE, beta=FAKE, running_mean=FAKE, running_var=FAKE, momentum=0.1, eps=1e-5,
               save_mean=FAKE, save_invstd=FAKE, y=FAKE, reps=2, zero_rows_per_row=1)
BN_REFUSALS = [dict(m=0), dict(m=-2), dict(c=0), dict(c=-1), dict(reps=0), dict(reps=-1), dict(zero_rows_per_row=-1),
               dict(m=1, reps=1, zero_rows_per_row=0)] + \
              [{k: None} for k in ("x", "gamma", "beta", "save_mean", "save_invstd", "y")]


def _bn_rep(**kw):
    a = dict(BN_GOOD)
    a.update(kw)
    return L.lib().tspm_bn1d_fwd_rep(a["m"], *[a[k] for k in BN_KEYS], None)


def _bn_rep_pair(first, second):
    a, b = dict(BN_GOOD), dict(BN_GOOD)
    a.update(first)
    b.update(second)
    m = first.get("m", second.get("m", BN_GOOD["m"]))
    return L.lib().tspm_bn1d_fwd_rep_pair(m, *[a[k] for k in BN_KEYS], *[b[k] for k in BN_KEYS], None)


@pytest.mark.parametrize("bad", BN_REFUSALS, ids=_ids(BN_REFUSALS))
def test_bn1d_fwd_rep_refusals(bad):
    """TSPM_ERR_INVALID with pointers no launch could survive and no device in the process: nothing was launched.  The
    pair form refuses the same argument in either half."""
    assert _bn_rep(**bad) == INVALID
    assert _bn_rep_pair(bad, {}) == INVALID
    assert _bn_rep_pair({}, bad) == INVALID


def test_bn1d_fwd_rep_one_row_is_enough_with_replication():
    """m = 1 is a valid batch as soon as the replicated batch has two rows: only the NULL output stops these."""
    for reps, zr in ((2, 0), (1, 1), (1, 2)):
        assert _bn_rep(m=1, reps=reps, zero_rows_per_row=zr, y=None) == INVALID
        assert _bn_rep(m=1, reps=reps, zero_rows_per_row=zr, running_mean=None, running_var=None, y=None) == INVALID


# ------------------------------------------------------------------------------------------------
# tspm_gmu_pattern_bwd
# ------------------------------------------------------------------------------------------------
GMU_GOOD = dict(batch=5, npat=3, keep=[1, 1, 1, 0, 0, 1], d=68, dz=FAKE, lddz=68, h=FAKE, ldh=136, gate=FAKE, wz=FAKE,
                du=FAKE, lddu=136, ds=FAKE, workspace=FAKE, workspace_bytes=1 << 30)
GMU_REFUSALS = [dict(batch=0), dict(batch=-3), dict(npat=0), dict(npat=L.MAX_PATTERNS + 1, keep=[1, 1] * (L.MAX_PATTERNS + 1)),
                dict(d=0), dict(d=-4), dict(d=L.GMU_PATTERN_MAX_D + 1, lddz=L.GMU_PATTERN_MAX_D + 1,
                                            ldh=2 * L.GMU_PATTERN_MAX_D + 2, lddu=2 * L.GMU_PATTERN_MAX_D + 2),
                dict(keep=[1, 1, 0, 0, 0, 1]), dict(lddz=67), dict(ldh=135), dict(lddu=135)] + \
               [{k: None} for k in ("keep", "dz", "h", "gate", "wz", "du", "ds")]


def _gmu_bwd(**kw):
    a = dict(GMU_GOOD)
    a.update(kw)
    keep = None if a["keep"] is None else (ctypes.c_int32 * len(a["keep"]))(*a["keep"])
    return L.lib().tspm_gmu_pattern_bwd(a["batch"], a["npat"], keep, a["d"], a["dz"], a["lddz"], a["h"], a["ldh"],
                                        a["gate"], a["wz"], a["du"], a["lddu"], a["ds"], a["workspace"],
                                        a["workspace_bytes"], None)


@pytest.mark.parametrize("bad", GMU_REFUSALS, ids=_ids(GMU_REFUSALS))
def test_gmu_pattern_bwd_refusals(bad):
    assert _gmu_bwd(**bad) == INVALID


def test_gmu_pattern_bwd_workspace():
    """One [2d] partial per workgroup, one workgroup per sample up to the forward's grid cap of 1024; a refused shape
    asks for nothing; a missing or short workspace is its own status, after the argument checks."""
    ws = L.lib().tspm_gmu_pattern_bwd_workspace
    assert ws(5, 68) == 5 * 2 * 68 * 4
    assert ws(1, 4) == 32
    assert ws(1024, 512) == ws(5000, 512) == 1024 * 2 * 512 * 4
    assert ws(0, 68) == ws(5, 0) == ws(5, L.GMU_PATTERN_MAX_D + 1) == 0
    need = ws(GMU_GOOD["batch"], GMU_GOOD["d"])
    assert _gmu_bwd(workspace=None) == WORKSPACE
    assert _gmu_bwd(workspace_bytes=need - 1) == WORKSPACE
    assert _gmu_bwd(workspace_bytes=0) == WORKSPACE
    assert _gmu_bwd(workspace=None, du=None) == INVALID  # an invalid argument wins over the workspace


# ------------------------------------------------------------------------------------------------
# the constructor, before anything touches a device
# ------------------------------------------------------------------------------------------------
def _cpu_model():
    torch.manual_seed(0)
    return M.MMIMDb(M.MMIMDbModalityEncoder(8, 8), M.MMIMDbModalityEncoder(8, 8),
                    M.GatedBiModalNetwork(8, 8, 8, 8), classifier=M.MLPGenreClassifier(8, 2, 8))


def test_constructor_refusals():
    model = _cpu_model()
    adam = torch.optim.Adam(model.parameters())
    with pytest.raises(L.TspmError, match="allreduce"):
        M.FusedMMIMDbPatternStep(model, adam, None, 4, allreduce=lambda: None)
    for bad in (["x"], ["it", "ti"], [], ["i", "i"]):
        with pytest.raises(ValueError):
            M.FusedMMIMDbPatternStep(model, adam, None, 4, patterns=bad)
    with pytest.raises(ValueError, match="fusion"):
        M.FusedMMIMDbPatternStep(model, adam, None, 4, fusion="triton")
    for pats, name in ((("t",), "image"), (("i",), "text")):  # the input BN of a never-kept modality has reps = 0
        with pytest.raises(L.TspmError, match=name):
            M.FusedMMIMDbPatternStep(model, adam, None, 4, patterns=pats)
    with pytest.raises(L.TspmError, match="FusedAdam"):
        M.FusedMMIMDbPatternStep(model, adam, None, 4)
    with pytest.raises(L.TspmError, match="FusedAdam"):
        M.FusedMMIMDbPatternStep(model, adam, None, 4, patterns=("t", "it"), fusion="launches")


def test_pattern_step_for_normalises_its_key():
    """The cache key holds the normalised pattern names: a bad selection raises before any step is built."""
    model = _cpu_model()
    with pytest.raises(ValueError):
        model.pattern_step_for(None, None, 4, patterns=["it", "x"])
    with pytest.raises(L.TspmError, match="FusedAdam"):
        model.pattern_step_for(torch.optim.Adam(model.parameters()), None, 4)
    assert not model.__dict__.get("_pattern_steps")
