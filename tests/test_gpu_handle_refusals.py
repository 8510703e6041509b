"""The table of tests/test_handle_refusals.py on the device path (capacity 8,
three admitted entries), and the one sequence whose state lives in the handle's
log commitment (csrc/log_commit.h): commit, reserve, commit again, cast one more
and commit, receipts and roots_at, on a fresh handle and on one restored with
and without an expected root."""
import pytest

from test_handle_refusals import ADMITTED, CAPACITY, CASES, IDS, NULLIFIERS, Box, Env, Ledger, check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def envs(ctx):
    return {kind: Env(kind, ctx) for kind in (Box, Ledger)}


@pytest.mark.parametrize("kind,name,call,rc,text", CASES, ids=IDS)
def test_refusal_on_the_device(envs, kind, name, call, rc, text):
    check_case(envs[kind], call, rc, text)


def admitted(kind, ctx):
    h = kind.open(ctx)
    h.cast_public(kind.pis(NULLIFIERS[:ADMITTED]), reserve=False)
    return h


def restored(kind, ctx, with_root):
    src = admitted(kind, None)
    root = src.commit_log()[0] if with_root else None
    if kind is Box:
        from ballot_model import PROPOSAL, ROOT_A
        return type(src).restore(ctx, PROPOSAL, [ROOT_A], src.entries(), capacity=CAPACITY, root=root)
    from ledger_model import ROOT_A
    return type(src).restore(ctx, [ROOT_A], src.entries(), capacity=CAPACITY, root=root)


@pytest.mark.parametrize("how", ["fresh", "restored", "restored_with_root"])
@pytest.mark.parametrize("kind", [Box, Ledger], ids=["box", "ledger"])
def test_commit_reserve_commit(ctx, kind, how):
    dev = admitted(kind, ctx) if how == "fresh" else restored(kind, ctx, how == "restored_with_root")
    host = admitted(kind, None)
    assert (dev.admitted, dev.capacity) == (ADMITTED, CAPACITY)
    first = dev.commit_log()
    assert first == host.commit_log() and first[1] == ADMITTED
    dev.reserve(17)
    assert dev.capacity == 17 and dev.commit_log() == first  # the tree was dropped; the rebuilt one has the same root
    for h in (dev, host):
        h.cast_public(kind.pis(NULLIFIERS[:4])[3:], reserve=False)
    assert dev.commit_log() == host.commit_log() and dev.commit_log()[1] == ADMITTED + 1
    for r in dev.receipts([0, 3]):
        assert (r.root, r.n) == dev.commit_log() and type(dev).check_receipt(r)
    assert dev.roots_at([3]) == [first[0]]
