"""GPU parity on the selector's decision boundaries: every case of tests/select_cases.py (the rows where a decision of
choose_compressor flips, and the pages that sit on the limits of the run-level kernel) is encoded on the device; PageMeta,
page codecs and page bytes must be the CPU oracle's.  tests/test_select_boundaries.py proves, without a GPU, that the
cases sit where they claim.

One test per family; the columns of a family that share their options go through one encode_columns call, and every
family runs twice on its context (the second call runs on the first one's launch hints)."""
from collections import OrderedDict

import pytest

from oracle import sbo as S
from tests import select_cases as T
from tests.test_gpu_encode import to_device_column, write_options
from tests.test_gpu_select import check

pytestmark = pytest.mark.gpu

FAMILIES = T.families()


def device_codecs(col, enc):
    try:
        return T.names(S.stat_column(col["ptype"], col["nullable"], enc.pages_numpy(), enc.metas_array())[0])
    except S.OracleError as e:
        return "pages the oracle cannot parse (%s)" % e


def run_family(ctx, cases, label=""):
    from strawboat_amd import write
    groups = OrderedDict()
    for c in cases:
        groups.setdefault(T.opt_key(c.opt), []).append(c)
    dev = {c.name: to_device_column(ctx, c.col) for c in cases}
    for rep in range(2):
        chose, failed = {}, []
        for group in groups.values():
            encs = write.encode_columns(ctx, [dev[c.name] for c in group], write_options(**group[0].opt))
            ctx.synchronize()
            for c, enc in zip(group, encs):
                chose[c.name] = device_codecs(c.col, enc)
                try:
                    check(ctx, c.col, enc=enc, **c.opt)
                except (AssertionError, S.OracleError) as e:     # (pages the oracle cannot parse raise inside check)
                    failed.append((c, str(e).split("\n")[0]))
        report = []
        for c, why in failed:
            line = "%s: device chose %s, oracle chose %s (%s)" % (c.name, chose[c.name], T.names(c.expect), why)
            if c.neighbour in chose:
                line += "; its neighbour %s: device chose %s, oracle chose %s" % (
                    c.neighbour, chose[c.neighbour], T.names(T.CASES[c.neighbour].expect))
            report.append(line)
        assert not report, "%scall %d, %d of %d cases:\n%s" % (label, rep + 1, len(report), len(cases), "\n".join(report))


@pytest.mark.parametrize("family", [f for f in FAMILIES if f not in T.FUSED_FAMILIES])
def test_boundaries(gpu_ctx, family):
    run_family(gpu_ctx, FAMILIES[family])


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("family", T.FUSED_FAMILIES)
def test_boundaries_of_the_fused_page_kernels_and_of_the_kernel_chain(family, fused, monkeypatch):
    """Dict pages of 2- / 4-byte integers and binary pages: selected by one workgroup per page (k_enc_prim_dict /
    k_enc_bin_page), or with SB_BIN_FUSED=0 (read when the context is created) by the chain of kernels"""
    import strawboat_amd as sb
    monkeypatch.setenv("SB_BIN_FUSED", fused)
    ctx = sb.Context(0)
    try:
        run_family(ctx, FAMILIES[family], "SB_BIN_FUSED=%s, " % fused)
    finally:
        ctx.close()
