"""What a context reports about its passes, by lifetime (mashmap_amd/csrc/mm_pass_state.h): the figures of mm_pass_stats, mm_result_counts
and mm_pass_redo_cause belong to the last mm_map_fragments and to nothing older; the four getters "as of the last sized pass" keep their
values over the steady-state passes behind it; the totals belong to the context.  A used context must report for a batch what a fresh one
does -- apart from the host waits, which depend on the buffers it already has."""
import pytest

import mmutil as U

pytestmark = pytest.mark.gpu

K, L, S, PI = 16, 1000, 32, 0.95
REF = U.random_dna(9301, 300000)


def reads_of(seed, n): return [a[:L].copy() for _, a, _ in U.sample_reads([REF], seed, n, L + 60, 0.02)]


@pytest.fixture(scope="module")
def batches():
    return reads_of(9302, 2000), reads_of(9303, 2500)                             # B: a quarter more reads than A, sized without a steady attempt


def make_ctx():
    from mashmap_amd import capi
    c = capi.Context(k=K, segLength=L, sketchSize=S, flags=capi.MM_FLAG_HG_FILTER)
    c.index_build([REF], kmerPct=0.0); c.set_tables_default(PI)
    return c


def sized_getters(c):
    return dict(l1_literal=c.pass_l1_literal(), group_fused=c.pass_l1_group_fused(), l2_window=c.pass_l2_window(), l2_large=c.pass_l2_large())


def every_getter(c):
    """all a context reports about its last pass, without the host waits and the totals"""
    return dict(sized_getters(c), steady=c.pass_stats()[1], counts=c.pass_counts(), results=c.result_counts(), cause=c.pass_redo_cause(),
                mappings=len(c.mappings()))


@pytest.fixture(scope="module")
def used(batches):
    """a context that has mapped A twice, with what it reported after each pass"""
    A, _ = batches
    c = make_ctx()
    assert c.reads_upload(A) == len(A)
    c.map(); first = dict(every_getter(c), waits=c.pass_stats()[0], totals=c.pass_totals())
    c.map(); second = dict(every_getter(c), waits=c.pass_stats()[0], totals=c.pass_totals())
    yield c, first, second
    c.close()


def test_a_steady_pass_reports_its_own_counts_and_the_sized_pass_s_figures(used):
    c, first, second = used
    assert not first["steady"] and first["waits"] > 1 and first["counts"]["l1"] > 0 and first["counts"]["l2"] > 0, first
    assert (second["waits"], second["steady"]) == (1, True), second
    assert second["counts"]["l1"] == first["counts"]["l1"] and second["counts"]["l2"] == first["counts"]["l2"] and second["results"] == first["results"]
    assert second["results"] == (first["counts"]["l1"], first["counts"]["l2"])
    for g in ("l1_literal", "group_fused", "l2_window", "l2_large"):
        assert second[g] == first[g], (g, first[g], second[g])
    assert first["totals"] == {"passes": 1, "steady": 0, "redone": 0} and second["totals"] == {"passes": 2, "steady": 1, "redone": 0}
    assert first["cause"] == 0 and second["cause"] == 0


def test_a_used_context_reports_a_larger_batch_as_a_fresh_one_does(used, batches):
    c, _, _ = used
    A, B = batches
    fresh = make_ctx()
    assert fresh.reads_upload(B) == len(B)
    fresh.map(); want = every_getter(fresh); want_totals = fresh.pass_totals()
    fresh.close()
    assert want_totals == {"passes": 1, "steady": 0, "redone": 0} and not want["steady"] and want["counts"]["l1"] > 0
    assert len(B) > len(A) + len(A) // 10
    t0 = c.pass_totals()
    assert c.reads_upload(B) == len(B)
    c.map()
    got, t1 = every_getter(c), c.pass_totals()
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert t1 == {"passes": t0["passes"] + 1, "steady": t0["steady"], "redone": t0["redone"]}, (t0, t1)


def test_an_empty_batch_reports_nothing_of_the_pass_before_it(used):
    c, _, _ = used
    c.map()                                                                       # whatever is resident: the pass before the empty one has figures to leave behind
    before, t0 = c.pass_counts(), c.pass_totals()
    assert before["l1"] > 0 and before["stream_entries"] > 0
    assert c.reads_upload([]) == 0
    c.map()
    assert c.result_counts() == (0, 0)
    assert c.pass_counts() == dict(l1=0, l2=0, queued=0, stream_entries=0, hard=0), c.pass_counts()
    assert c.pass_redo_cause() == 0 and not c.pass_stats()[1]
    t1 = c.pass_totals()
    assert t1 == {"passes": t0["passes"] + 1, "steady": t0["steady"], "redone": t0["redone"]}, (t0, t1)
