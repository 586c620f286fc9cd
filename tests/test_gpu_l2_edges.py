"""The L2 stream kernels -- k_l2_extents, k_l2_locate, k_l2_sweep<narrow|wide>, k_l2_sweep_exact (mashmap_amd/csrc/mm_l2.hip) -- at the
edges of the stream format and of the counter ladder, on inputs built for each edge (tests/l2plant.py):

  skip entries      inserts of a slide, and the end marker, further apart than the delta field holds: 8191 at the 11-bit sketch-position field
                    (s = 3 and 5 over segments of 30 kbp), 2047 at the 13-bit one (s = 2100 and a hole in the index)
  tail loops        64 .. 127 and 128 and more evictions at the end of a slice (the look-back for the last insert), 64 and more behind it (the
                    look-ahead for the next insert), a slice behind which the contig has no insert
  bucket walk       every q[p] - 1, q[p] + 1, 0, qmax + 1 and 2^64 - 1 in the slide, at both field widths
  counter ladder    a cell of the slide at 31 | 32 and at 4095 | 4096, a pre-load cell at 31 | 32, a pre-load of 3999 | 4000 records at the
                    default limit

tests/test_l2_plant_model.py holds, without a GPU, that every input sits on its edge, and that two edges have no input: the first delta of
a stream is always 0 (no first_gap, no slide without an insert).  A gap beyond 2^27 (the bigSkip branch of k_l2_locate) is not covered.

Every case goes through gpucheck.run_and_compare over the planted index: the sized, the steady-state and the HBM-point pass against the
oracle on every integer (the steady-state pass is the one with the fixed-capacity wide and exact launches).  The ladder cases then count
the sweep launches of one more sized pass on a fresh context: 1 = narrow, 2 = narrow and wide, 3 = narrow, wide and exact."""
import pytest

import gpucheck
import l2plant as P
import mmutil as U

pytestmark = pytest.mark.gpu


def compare(oracle, c):
    return gpucheck.run_and_compare(oracle, c["contigs"], c["reads"], k=c["k"], L=c["L"], s=c["s"], pi=c["pi"], flags=c["flags"], kmerPct=0.0,
                                    check_points=False, mutate_index=c["mutate"])


def sweep_launches(oracle, c):
    """(launches of the L2 sweep kernels, brackets around k_l2_extents and k_l2_locate) of a sized pass on a fresh context"""
    from mashmap_amd import capi
    h = oracle.session(c["contigs"], c["k"], c["L"], c["s"], c["pi"], U.FILTER_MAP, c["flags"], b"\0", 0.0, mutate_index=c["mutate"])
    ix = oracle.export_index(h)
    ctx = capi.Context(k=c["k"], segLength=c["L"], sketchSize=c["s"], flags=capi.MM_FLAG_HG_FILTER if c["flags"] & U.FLAG_HG else 0)
    ctx.index_upload(ix["minmers"], ix["keys"], ix["offsets"], ix["points"], ix["freq"], ix["contigLen"])
    ctx.set_tables(oracle.min_hits_table(c["s"], c["k"], c["pi"]), oracle.cutoffs(h))
    ctx.reads_upload([a for _, a in c["reads"]])
    ctx.profile(True); ctx.profile_read(reset=True)
    ctx.map()
    prof = ctx.profile_read()
    n1 = ctx.result_counts()[0]
    ctx.close(); oracle.free(h)
    assert n1 == len(c["facts"])
    return prof["l2"][1], prof["l2_locate"][1]


@pytest.mark.parametrize("name", ["skip_jb11_s3", "skip_jb11_s5", "skip_jb13", "tail_and_behind", "last_of_contig", "hash_neighbours_s130", "hash_neighbours_s2100"])
def test_stream_edges(oracle, name):
    c = P.CASES[name]()
    nF, nl = compare(oracle, c)
    assert nF == len(c["reads"]) and nl >= 1
    sweeps, locates = sweep_launches(oracle, c)
    assert (sweeps, locates) == (1, 2), "not one chunk through the narrow sweep alone: %r" % ((sweeps, locates),)


@pytest.mark.parametrize("name", ["cell_31", "cell_32", "cell_4095", "cell_4096", "preload_cell_31", "preload_cell_32", "preload_3999", "preload_4000"])
def test_counter_ladder(oracle, name):
    c = P.CASES[name]()
    nF, nl = compare(oracle, c)
    assert nF == 1 and nl >= 1
    sweeps, locates = sweep_launches(oracle, c)
    assert locates == 2, "the batch was not located once, in one chunk: %d" % locates
    assert sweeps == c["launches"], "%s: %r takes %d sweep launches, the sized pass had %d" % (name, c["facts"][0]["route"], c["launches"], sweeps)
