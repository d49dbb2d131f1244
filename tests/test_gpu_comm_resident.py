"""-m gpu: aln_gather_resident_enqueue / _collect (Comm.gather_enqueue / gather_collect) on the one GPU the box has, through a
1-rank RCCL communicator like tests/test_gpu_comm.py: the scores go from the batch's resident results into the collective and
come back through one of two pinned slots.  Comm.gather (aln_gather_scores) over the host copy of the same scores is the
reference; every comparison is bit-exact.  The N > 1 branch has, like aln_gather_scores', no hardware to run on here."""
import numpy as np
import pytest

import aln_amd
import gpu_util
from aln_amd.shard import Comm, deal_units, local_units

pytestmark = pytest.mark.gpu

N = 9


@pytest.fixture(scope="module")
def job():
    """Nine pairs of 40-100 residues, dealt over one rank (longest first)."""
    from aln_amd.synth import random_pair
    pairs = [random_pair(47000 + n, 40 + 7 * n, 100 - 5 * n) for n in range(N)]
    work = [(len(q) + 2) * (len(t) + 2) for q, t in pairs]
    owner, slot = deal_units(work, 1)
    mine = local_units(owner, slot, 0)
    assert sorted(mine.tolist()) == list(range(N))
    return pairs, mine


def make_batch(ctx, job):
    pairs, mine = job
    return aln_amd.Batch(ctx, [pairs[k][0] for k in mine], [pairs[k][1] for k in mine])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def raises(code, fn, *args, **kw):
    with pytest.raises(aln_amd.AlnError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value


def round_trip(comm, b, mine, want):
    """A successful enqueue / collect: also the proof that whatever came before left no slot occupied (a third pending
    enqueue, or a collect of someone else's slot, would show here)."""
    b.optimal_enqueue()
    comm.gather_enqueue(b, mine, N, N)
    out = comm.gather_collect(N)
    assert np.array_equal(bits(out[mine]), bits(want))
    raises(aln_amd.E_STATE, comm.gather_collect, N)        # ... and exactly one was pending
    got, _, status = b.optimal_collect()
    assert (status == 0).all() and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("mode", [aln_amd.LOCAL, aln_amd.GLOBAL], ids=["local", "global"])
def test_parity_with_the_host_path(blosum62, job, mode):
    alpha, table = blosum62
    pairs, mine = job
    ctx = gpu_util.ctx()
    b = make_batch(ctx, job)
    comm = Comm(ctx, 1, 0)
    b.dp_submatrix(alpha, table, mode, 11, 1)
    b.optimal_enqueue()
    comm.gather_enqueue(b, mine, N, N)
    out = comm.gather_collect(N)
    want, _, status = b.optimal(want_pairs=False)
    assert (status == 0).all()
    assert np.array_equal(bits(out[mine]), bits(want))
    assert np.array_equal(bits(out), bits(comm.gather(want, mine, N, N)))
    # the batch's own slot pair is independent of the communicator's: its pending collect still delivers
    got, _, status = b.optimal_collect()
    assert (status == 0).all() and np.array_equal(bits(got), bits(want))
    comm.close()
    b.close()


def test_oldest_first_two_slots(blosum62, job):
    alpha, table = blosum62
    pairs, mine = job
    ctx = gpu_util.ctx()
    b = make_batch(ctx, job)
    comm = Comm(ctx, 1, 0)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 8, 2)
    s82 = b.optimal(want_pairs=False)[0].copy()
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    s111 = b.optimal(want_pairs=False)[0].copy()
    assert not np.array_equal(s82, s111)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    b.optimal_enqueue()
    comm.gather_enqueue(b, mine, N, N)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 8, 2)
    b.optimal_enqueue()
    comm.gather_enqueue(b, mine, N, N)
    raises(aln_amd.E_STATE, comm.gather_enqueue, b, mine, N, N)     # both slots are waiting
    assert np.array_equal(bits(comm.gather_collect(N)[mine]), bits(s111))
    assert np.array_equal(bits(comm.gather_collect(N)[mine]), bits(s82))
    raises(aln_amd.E_STATE, comm.gather_collect, N)
    assert np.array_equal(bits(b.optimal_collect()[0]), bits(s111))
    assert np.array_equal(bits(b.optimal_collect()[0]), bits(s82))
    comm.close()
    b.close()


def test_padding_and_untouched_positions(blosum62, job):
    alpha, table = blosum62
    pairs, mine = job
    ctx = gpu_util.ctx()
    b = make_batch(ctx, job)
    comm = Comm(ctx, 1, 0)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    want = b.optimal(want_pairs=False)[0]
    total = 12

    def partial(index):
        comm.gather_enqueue(b, index, N, total)
        out = comm.gather_collect(total, out=np.full(total, -7, np.float32))
        rest = np.setdiff1d(np.arange(total), index)
        assert np.array_equal(bits(out[index]), bits(want[:len(index)])) and len(rest) == total - len(index)
        assert (out[rest] == -7).all()

    for rep in range(3):                                   # buffers and the cached index list are reused
        partial(mine[:4])
    # a rank with nothing to contribute sends padding only
    comm.gather_enqueue(None, np.zeros(0, np.int32), 5, total)
    out = comm.gather_collect(total, out=np.full(total, -7, np.float32))
    assert (out == -7).all()
    partial(mine[:4])
    other = (mine[:4] + 3).astype(np.int32)                # same length, other positions (up to 11): the cache must notice
    assert not np.array_equal(other, mine[:4])
    partial(other)
    partial(mine[:4])
    comm.close()
    b.close()


def test_state_and_argument_errors_leave_no_slot_occupied(blosum62, job):
    alpha, table = blosum62
    pairs, mine = job
    ctx = gpu_util.ctx()
    b = make_batch(ctx, job)
    comm = Comm(ctx, 1, 0)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    raises(aln_amd.E_STATE, comm.gather_enqueue, b, mine, N, N)          # no Optimal launched on this build
    want = b.optimal(want_pairs=False)[0].copy()
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    raises(aln_amd.E_STATE, comm.gather_enqueue, b, mine, N, N)          # ... and a rebuild invalidates the one before
    round_trip(comm, b, mine, want)
    ctx2 = aln_amd.Context(0)                                            # a second context of the same device
    b2 = make_batch(ctx2, job)
    b2.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    assert np.array_equal(bits(b2.optimal(want_pairs=False)[0]), bits(want))
    raises(aln_amd.E_ARG, comm.gather_enqueue, b2, mine, N, N)
    b2.close()
    ctx2.close()
    bad = mine.copy()
    bad[5] = N
    raises(aln_amd.E_ARG, comm.gather_enqueue, b, bad, N, N)             # index == n_total
    bad[5] = -1
    raises(aln_amd.E_ARG, comm.gather_enqueue, b, bad, N, N)
    raises(aln_amd.E_ARG, comm.gather_enqueue, b, mine, 4, N)            # n_local > n_max
    raises(aln_amd.E_STATE, comm.gather_collect, N)                      # none of them enqueued anything
    comm.gather_enqueue(b, mine, N, N)
    raises(aln_amd.E_STATE, comm.gather_collect, N + 1)                  # not the n_total it was enqueued with: the slot is dropped
    raises(aln_amd.E_STATE, comm.gather_collect, N)
    b.reevaluate()
    round_trip(comm, b, mine, want)
    comm.close()
    b.close()


def test_destroy_with_work_pending(blosum62, job):
    alpha, table = blosum62
    pairs, mine = job
    ctx = gpu_util.ctx()
    b = make_batch(ctx, job)
    comm = Comm(ctx, 1, 0)
    b.dp_submatrix(alpha, table, aln_amd.LOCAL, 11, 1)
    want = b.optimal(want_pairs=False)[0].copy()
    comm.gather_enqueue(b, mine, N, N)
    comm.close()                                                         # never collected
    got, _, status = b.optimal(want_pairs=False)
    assert (status == 0).all() and np.array_equal(bits(got), bits(want))
    b.close()
