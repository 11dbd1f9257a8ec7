"""tspm_regress_head_step refuses every argument outside its limits with TSPM_ERR_INVALID before any launch (no GPU
needed: an accepted call would answer TSPM_ERR_LAUNCH = 2 here)."""
import ctypes

from tspm_amd import _lib as L

INVALID = 1
P = 4096  # a 16-byte aligned, non-NULL stand-in: never dereferenced, every call returns before a launch


def _call(train=True, **kw):
    f = dict(n=128, hid=32, ld_emb=32, ld_demb=32, kind=L.REGRESS_L1, n_groups=1, loss_weight=1.0, emb=P, w=P, b=P,
             labels=P, groups=None, pred=P, loss=P, dw=P if train else None, db=P if train else None,
             demb=P if train else None, stats=None, loss_log=None, counters=None, log_capacity=0)
    f.update(kw)
    return L.load().tspm_regress_head_step(ctypes.byref(L.RegressHeadDesc(**f)), None)


def test_regress_head_limits_are_refused_before_launch():
    assert L.load().tspm_regress_head_step(None, None) == INVALID
    assert _call(n=0) == INVALID and _call(n=1025) == INVALID and _call(n=-3) == INVALID
    assert _call(hid=0) == INVALID and _call(hid=132, ld_emb=132, ld_demb=132) == INVALID
    assert _call(hid=30, ld_emb=32) == INVALID  # not a multiple of 4
    assert _call(ld_emb=28) == INVALID and _call(ld_emb=34) == INVALID
    assert _call(ld_demb=28) == INVALID and _call(ld_demb=34) == INVALID
    assert _call(emb=P + 4) == INVALID and _call(demb=P + 8) == INVALID  # 16-byte alignment
    assert _call(kind=2) == INVALID and _call(kind=-1) == INVALID
    for missing in ("emb", "w", "b", "labels", "pred", "loss"):
        assert _call(**{missing: None}) == INVALID, missing
    # the whole backward or none of it
    assert _call(dw=None) == INVALID and _call(db=None) == INVALID and _call(demb=None) == INVALID
    assert _call(train=False, dw=P) == INVALID
    # accumulators: 1 .. 16 groups; the loss log needs the counters
    assert _call(stats=P, n_groups=0) == INVALID and _call(stats=P, n_groups=17) == INVALID
    assert _call(stats=P + 4, n_groups=1) == INVALID
    assert _call(loss_log=P) == INVALID and _call(counters=P, log_capacity=-1) == INVALID


def test_regress_head_binding_matches_the_header_struct():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tspm.h")).read()
    body = re.search(r"typedef struct tspm_regress_head_desc \{(.*?)\} tspm_regress_head_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[-1].replace("float*", "").replace("int32_t*", "")
             .replace("int64_t*", "").replace("tspm_regress_stats*", "").replace("float", "").replace("int32_t", "")
             .replace("int64_t", "").split(",")]
    assert names == [n for n, _ in L.RegressHeadDesc._fields_]
    assert ctypes.sizeof(L.RegressHeadDesc) == 8 * 4 + 13 * 8 + 8
    assert "typedef struct tspm_regress_stats" in hdr and L.REGRESS_STATS_WORDS * 8 == 8 + 7 * 8 + 49 * 8 + 9 * 8
