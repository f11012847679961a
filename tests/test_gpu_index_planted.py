"""The seen-chunk index (backuwup_amd/csrc/bw_dedup.hip: k_append_claim, k_verdict, k_rehash, and
index_capacity() of bw_capi.hip) on the planted cases of tests/index_plant.py.

Every other index test draws random digests, with which a tag match is a true duplicate: nothing
after the tag compare decides, no probe run wraps, no table word is 0 or carries the tag 0xffffff,
and a rehash never rebuilds a probe cluster.  The cases here plant all of that (the census each one
produces is checked on the CPU by tests/test_index_plant.py, with the mutants it catches), and run
through every entrance that reaches launch_dedup: the host form (with bw_index_seed where the case
has a seed), the device form, and the exchange's bucket form with 1 and 8 sources.

Each test has a context of its own: the capacity must be a fresh context's 65 536 slots, so that
`grow` crosses exactly the growths the capacity rule predicts.  After every batch the verdicts equal
the plain duplicate rule exactly, bw_index_size equals the distinct count, bw_index_check is clean
(no lookup without a slot), and canaries and guards are untouched.
"""
import contextlib

import numpy as np
import pytest

import index_plant as P

pytestmark = pytest.mark.gpu

V_CANARY = 7          # verdict bytes before the call
GUARD = 64            # bytes behind every verdict buffer that must stay untouched
ENTRANCES = ("host", "device", "buckets1", "buckets8")


@contextlib.contextmanager
def fresh_context(reset_hint=None):
    """A new context on a torch stream of its own (uploads, the library's kernels and the read-backs
    are ordered on it)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from backuwup_amd import Context
    st = torch.cuda.Stream()
    c = Context(0)
    try:
        c.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            if reset_hint is not None:
                c.index_reset(reset_hint)
            yield torch, c
            st.synchronize()
    finally:
        c.close()


def up(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cases' arrays are read-only


def not_yet_seen(name, b):
    """Digests that are not part of batches 0..b of the case and would change a later verdict or the
    distinct count if a slot holding one were gated: first occurrences of the later batches (at most
    64), and planted cluster members that no batch holds."""
    _, batches = P.case(name)
    want_v, _ = P.expected(name)
    later = [batches[k][want_v[k] == 0][:32] for k in range(b + 1, min(b + 3, len(batches)))]
    fill = np.concatenate(later + [P.decoys()])
    seen = {x.tobytes() for k in range(b + 1) for x in batches[k]}
    assert not any(x.tobytes() in seen for x in fill)
    return fill


def gate(torch, c, entrance, name, b):
    """Batch b of the case through one entrance -> its verdicts (canaries and guards checked)."""
    batch = P.case(name)[1][b]
    n = len(batch)
    if entrance == "host":
        return c.index_check_insert(batch)
    if entrance == "device":
        d = up(torch, batch)
        v = torch.full((n + GUARD,), V_CANARY, dtype=torch.uint8, device="cuda")
        c.index_check_insert_device(d.data_ptr(), n, v.data_ptr())
        got = v.cpu().numpy()
        assert (got[n:] == V_CANARY).all(), (name, b, "guard")
        return got[:n]
    n_src = int(entrance[len("buckets"):])
    recv, counts, cap = P.buckets(batch, n_src, not_yet_seen(name, b))
    assert (counts < cap).all() and n_src * cap - n > 256  # *n_dev < max_n: the gate's last block is empty
    r, k = up(torch, recv), up(torch, counts)
    v = torch.full((n_src * cap + GUARD,), V_CANARY, dtype=torch.uint8, device="cuda")
    c.index_check_insert_buckets(r.data_ptr(), k.data_ptr(), n_src, cap, v.data_ptr())
    got = v.cpu().numpy()
    assert (got[n_src * cap:] == V_CANARY).all(), (name, b, "guard")
    slots = got[:n_src * cap].reshape(n_src, cap)
    live = np.arange(cap)[None, :] < counts[:, None]
    assert (slots[~live] == V_CANARY).all(), (name, b, "a verdict in a slot beyond its bucket's count")
    return slots[live]  # source-major: canonical order


def run_case(torch, c, name, entrance):
    """The whole case; the checks after every batch.  -> the verdicts."""
    seed, batches = P.case(name)
    want_v, want_n = P.expected(name)
    if seed is not None:
        c.index_seed(seed)
        assert c.index_size() == len(seed)
        c.index_check()
    out = []
    for b in range(len(batches)):
        got = gate(torch, c, entrance, name, b)
        bad = np.flatnonzero(got != want_v[b])
        assert bad.size == 0, "%s/%s batch %d: %d of %d verdicts differ, first at %s: got %s want %s" % (
            name, entrance, b, bad.size, len(got), bad[:8], got[bad[:8]], want_v[b][bad[:8]])
        assert c.index_size() == want_n[b], (name, entrance, b)
        c.index_check()
        out.append(got)
    return out


@pytest.mark.parametrize("entrance", ENTRANCES)
@pytest.mark.parametrize("name", tuple(P.CASES))
def test_planted_case(name, entrance):
    with fresh_context() as (torch, c):
        run_case(torch, c, name, entrance)


def test_grow_agrees_with_a_presized_index():
    """The same batches on an index that never grows (no rehash, no log copy): identical verdicts."""
    sizes = [len(b) for b in P.case("grow")[1]]
    assert len({t for t, _ in P.capacity_after(sizes)}) == 3                        # grows twice ...
    assert len({t for t, _ in P.capacity_after(sizes, reset_hint=P.PRESIZE)}) == 1  # ... and not at all
    with fresh_context() as (torch, c):
        grown = run_case(torch, c, "grow", "device")
    with fresh_context(P.PRESIZE) as (torch, c):
        flat = run_case(torch, c, "grow", "device")
    assert len(grown) == len(flat) and all(np.array_equal(g, f) for g, f in zip(grown, flat))
