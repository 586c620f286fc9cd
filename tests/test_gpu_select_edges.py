"""k_l2_select (mashmap_amd/csrc/mm_select.hip over mm_select_core.h and mm_heap.h), doL2Mapping's best-first walk with one thread per
fragment, on the planted inputs of tests/selplant.py:

  ties              2 .. 64 candidates of one intersectionSize: at an entry of the cut-off table that is best + 1 one of them is reported,
                    the one libstdc++'s std::make_heap brings to the front; at a plain entry all are, in heap order
  levels            ties at two and three levels; a locus that puts the cut between two lower levels
  acceptance        a locus at the first accepted count of its row and one below, with and without FLAG_DROP_LOW_ID
  rows              a fragment of Q.sketchSize 129 beside one of 130: the table's row is the fragment's, not the context's sketch size
  flags             no HG filter (candidate order); FLAG_SKIP_PREFIX (best starts again in every reference group; a read's own group)
  placement         fragments without candidates and without a sketch between the others; 257 fragments, ties in the last two
  many              1 000 candidates of one fragment

tests/test_select_walk.py holds on the CPU that every input sits on its edge.  Every case goes through gpucheck.run_and_compare over the
planted index -- the sized, the steady-state and the HBM-point pass against the oracle on every integer, the records as sorted lists --,
and then the device's records of every fragment, IN DEVICE ORDER, are held against the push sequence of walker (a): the float replay of
skch_map_post.hpp with std::make_heap / std::pop_heap (hl_select_walk, tests/hostlogic/hostlogic.cpp)."""
import pytest

import gpucheck
import selplant as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(P.CASES))
def test_select_edges(oracle, name):
    c = P.CASES[name]()
    maps = {}
    nF, nl = gpucheck.run_and_compare(oracle, c["contigs"], c["reads"], k=P.K, L=P.L, s=c["s"], pi=c["pi"], flags=c["flags"], delim=c["delim"],
                                      kmerPct=c["kmerPct"], mutate_index=c["mutate"], maps_out=maps)
    assert nF == len(c["reads"]) == len(maps) and nl == sum(len(fr["l2"]) for fr in c["per"])
    pushes = 0
    for f, fr in enumerate(c["per"]):
        want = P.pushed_records(fr, "a")
        assert maps[f] == want, "%s fragment %d: the device's records %r, the reference's push order %r" % (name, f, maps[f], want)
        pushes += len(want)
    print("%s: %d fragments, %d candidates, %d records in the reference's push order" % (name, nF, sum(len(fr["l1"]) for fr in c["per"]), pushes))
    assert pushes > 0
