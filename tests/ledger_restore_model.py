"""Reopening a transfer ledger from its published log, and payout rounds, as a
model, and the cases the host-path and the device tests both run.  Nothing in
the model calls the code under test.

Restore (include/qpgpu.h qp_ledger_restore) = the audit's reasons
1-3 (non-canonical, order, credit rule), and 6 (the root) when one is expected,
by ledger_log_model.audit; then a ledger_model.Model whose dicts are filled
from the log (model_from_log), with cast = cast_count.  Everything a ledger
shows afterwards is that Model's.

A payout round (qp_ledger_payouts_between): the accounts credited by the log
entries [m0, m1), each with the exact sum of its credited entries of the range
and the lowest such seq, in the order of that seq (payouts_between).
"""
import ctypes

import numpy as np

from ledger_log_model import (CREDIT_RULE, NON_CANONICAL, OK, ORDER, ROOT, LedgerLogModel, _edit, _swap_numbers,
                              amount_of, arrays_of, audit, log_of, sized_items)
from ledger_model import (MAX_AMOUNT, ROOT_A, Model, account_bytes, batches, cast_batch, check_against_model,
                          make_stream, transfer)
from oracle_lib import P

REPLAY_STRIDE = 97
EDGE_SIZES = [1, 2, 255, 256, 257, 513]


def model_from_log(roots, padding, log, cast_count):
    """the Model of a ledger that holds `log` ([(nullifier, number, limbs, account, flags)]) and has cast
    cast_count transfers: its dicts filled from the log, the flags trusted (the audit ran before)"""
    m = Model(roots, padding)
    m.cast = cast_count
    for seq, (nul, num, limbs, acc, fl) in enumerate(log):
        amount = amount_of(limbs)
        m.log.append((nul, num, amount, acc, bool(fl & 1)))
        m.seen.setdefault(nul, num)
        if fl & 1:
            m.seq_of[nul] = seq
            if acc not in m.totals:
                m.order.append(acc)
                m.first_seq[acc] = seq
            m.totals[acc] = m.totals.get(acc, 0) + amount
    return m


def restore_verdict(log, root=None):
    """(status, witness, first) of a restore of `log`: the audit with the root as its only claim; an empty
    log restores"""
    if not log:
        return OK, None, None
    rep = audit(log, root=root)
    assert rep.status in (OK, NON_CANONICAL, ORDER, CREDIT_RULE, ROOT)
    return rep.status, rep.witness, rep.first


def payouts_between(log, m0, m1):
    """[(account, exact total, first_seq)] of the credited entries of log[m0:m1], in first_seq order"""
    assert 0 <= m0 <= m1 <= len(log)
    totals, first = {}, {}
    for seq in range(m0, m1):
        _, _, limbs, acc, fl = log[seq]
        if fl & 1:
            first.setdefault(acc, seq)
            totals[acc] = totals.get(acc, 0) + amount_of(limbs)
    return [(acc, totals[acc], s) for acc, s in first.items()]  # dicts keep the order of first insertion


def rows(payouts):
    """the model's rows in the form WormholeLedger.payouts_between returns"""
    return [(account_bytes(a), t, s) for a, t, s in payouts]


def raw_entries(led):
    """the whole log as arrays (amounts as limbs), cheap to slice at a cut"""
    return led._entries_at(np.arange(led.admitted, dtype=np.uint64))


def restore(ctx, roots, entries, **kw):
    from qp_wormhole import WormholeLedger
    return WormholeLedger.restore(ctx, roots, entries, **kw)


# ---- restore at the cuts

def restore_cuts(name):
    """(steps, cuts, replayed) of stream `name` under batching 7: a restore is tried after every cast
    step in `cuts`; after those in `replayed` the restored ledger also casts the rest of the stream.  A
    stream of at most 40 batches is replayed from every cut; a longer one (many_blocks: 878 batches) from
    its first three cuts, its last three and every 97th, since each replay costs the rest of the stream;
    those are also the cuts at which a long stream's restore expects the root (check_restore_stream)."""
    steps = list(batches(make_stream(name)[3], 7))
    casts = [i for i, s in enumerate(steps) if s[0] == "cast"]
    if len(casts) <= 40:
        return steps, casts, set(casts)
    return steps, casts, set(casts[:3] + casts[-3:] + casts[::REPLAY_STRIDE])


def observe(led, nullifiers, accounts):
    """everything observable of a ledger after its stream"""
    from qp_wormhole import WormholeLedger
    nul, num, amt, acc, fl = raw_entries(led)
    out = [nul.tolist(), num.tolist(), amt.tolist(), acc.tolist(), fl.tolist(), led.payouts(), led.recount(),
           (led.cast_count, led.admitted, led.credited, led.accounts, led.capacity)]
    if led.admitted:
        out += [led.commit_log(), led.find(nullifiers), led.totals_for(accounts)]
        r = led.receipts([led.admitted - 1])[0]
        assert WormholeLedger.check_receipt(r)
        out.append(tuple(r))
    return out


def check_restore_stream(ctx, ledger_factory, name, entries_factory=None):
    """For each cut (restore_cuts): a ledger restored from the entries at the cut, with the root the log
    had there expected and the stream's padding, has the uninterrupted ledger's state, payouts, recount,
    `find` of every nullifier of the stream, totals and commitment of that point, all equal to the
    model's, and a receipt of its last entry equals the uninterrupted ledger's.  From the replayed cuts
    the Model filled from the log is held against everything observable, and the restored ledger casts
    the rest of the stream: statuses, `first`, the log, the payouts and commit_log() equal the
    uninterrupted ledger's.  entries_factory: the path whose ledger publishes the entries."""
    from qp_wormhole.ledger import NOT_FOUND
    cap0, roots, padding, items = make_stream(name)
    steps, cuts, replayed = restore_cuts(name)
    model = Model(roots, padding)
    led = (entries_factory or ledger_factory)(roots, padding, cap0)
    results, state, cap = [], [], cap0
    try:
        for kind, arg in steps:
            if kind == "reserve":
                led.reserve(arg)
                cap = arg
            else:
                results += [tuple(r) for r in cast_batch(led, arg)]
                assert results[-len(arg):] == [model.cast_one(pi, v) for pi, v in arg]
            want = ((model.cast, len(model.log), len(model.seq_of), len(model.order), cap), rows(model.payouts()),
                    (len(model.seq_of), len(model.log), sum(model.totals.values())))
            assert want == ((led.cast_count, led.admitted, led.credited, led.accounts, led.capacity), led.payouts(),
                            led.recount())
            state.append(want + (len(results),))
        nullifiers = [list(k) for k in model.seen]
        accounts = [list(a) for a in model.order]
        queries = np.array(nullifiers, dtype=np.uint64).reshape(len(nullifiers), 4)
        final = raw_entries(led)
        want_end = observe(led, nullifiers, accounts)
        final_find = led.find(queries, raw=True) if nullifiers else np.zeros(0, np.uint64)
        sizes = sorted({s[0][1] for s in state if s[0][1]})
        at_root = dict(zip(sizes, led.roots_at(sizes))) if sizes else {}
        last_receipt = {m: tuple(r) for m, r in zip(sizes, led.receipts([m - 1 for m in sizes]))} if sizes else {}
    finally:
        led.free()
    for c in cuts:
        (cast_count, admitted, credited, naccounts, cap), pay, recount, done = state[c]
        entries = tuple(a[:admitted] for a in final)
        # hashing the whole log at each of 878 cuts is what a long stream cannot afford within seconds: it
        # expects the root, commits and takes the receipt at the replayed cuts, and restores without a root
        # (reasons 1-3, both tables, the sums) at every other cut
        hashed = admitted and c in replayed
        again = restore(ctx, roots, entries, cast_count=cast_count, padding=padding, capacity=cap,
                        root=at_root[admitted] if hashed else None)
        try:
            assert (again.cast_count, again.admitted, again.credited, again.accounts, again.capacity) == state[c][0]
            assert again.payouts() == pay and again.recount() == recount, (name, c)
            if admitted:
                found = again.find(queries, raw=True)
                assert (found == np.where(final_find < admitted, final_find, np.uint64(NOT_FOUND))).all(), (name, c)
                assert again.totals_for([a for a, _, _ in pay]) == [t for _, t, _ in pay]
            if hashed:
                assert again.commit_log() == (at_root[admitted], admitted), (name, c)
                # the receipt under (root, admitted): the uninterrupted ledger's path at its final size differs
                r = again.receipts([admitted - 1])[0]
                assert (r.root, r.n, r.seq) == (at_root[admitted], admitted, admitted - 1)
                if admitted == sizes[-1]:
                    assert tuple(r) == last_receipt[admitted]
            if c not in replayed:
                continue
            log = log_of((entries[0], entries[1], [amount_of(a) for a in entries[2]], entries[3], entries[4]))
            if admitted <= 600:  # the model hashes in Python; the roots of longer logs are test_ledger_log.py's
                assert restore_verdict(log, at_root.get(admitted)) == (OK, None, None)
            check_against_model(again, model_from_log(roots, padding, log, cast_count), cap)
            rest = [it for s in steps[c + 1:] for it in (s[1] if s[0] == "cast" else [s])]
            got = []
            for kind, arg in batches(rest, None):
                if kind == "reserve":
                    again.reserve(arg)
                else:
                    got += [tuple(r) for r in cast_batch(again, arg)]
            assert got == results[done:], (name, c)
            assert observe(again, nullifiers, accounts) == want_end, (name, c)
        finally:
            again.free()
    return want_end


# ---- block edges

def edge_items(n):
    """n transfers to 5 accounts whose double spends come in runs that cross the edges of the 256-lane
    blocks and of the 64-lane waves: entries 60..69 and 250..262 and 508..512 repeat entry 3, 7 or an
    entry just before the run"""
    items = sized_items(n, seed=5000 + n)
    for lo, hi, first in ((60, 70, 3), (250, 263, 7), (508, 513, 249)):
        for i in range(lo, min(hi, n)):
            items[i] = (transfer(items[first][0][0:4], 100 + i, items[i][0][12:16]), 0)
    return items


def check_block_edges(ctx, ledger_factory, n):
    """a log of n entries restored at capacity exactly n (the next admitted cast is refused, then
    reserve, then it is accepted), at 2 n + 3, and restore, reserve, cast; each holds the Model filled
    from the log"""
    import pytest
    from qp_wormhole import QpError
    items = edge_items(n)
    led = ledger_factory([ROOT_A], None, n)
    try:
        cast_batch(led, items)
        entries, (root, got_n) = led.entries(), led.commit_log()
        pay = led.payouts()
    finally:
        led.free()
    assert got_n == n
    log = log_of(entries)
    assert restore_verdict(log, root) == (OK, None, None)
    new = (transfer([7, 7, 7, 7], 5, [1, 2, 3, 4]), 0)
    out = []
    for cap, reserve_first in ((n, False), (2 * n + 3, False), (n, True)):
        model = model_from_log([ROOT_A], None, log, 2 * n)
        again = restore(ctx, [ROOT_A], entries, cast_count=2 * n, capacity=cap, root=root)
        try:
            check_against_model(again, model, cap)
            assert again.payouts() == pay and again.commit_log() == (root, n)
            if cap == n and not reserve_first:
                with pytest.raises(QpError, match="QP_ERR_ARG.*capacity"):
                    cast_batch(again, [new])
                check_against_model(again, model, cap)  # a refused call leaves everything as it was
            if cap == n:
                again.reserve(n + 2)
                cap = n + 2
                check_against_model(again, model, cap)
            # a fresh transfer, then a double of an old credited entry and of an old double spend
            batch = [new, (transfer(items[0][0][0:4], 9, [1, 2, 3, 4]), 0)]
            got = [tuple(r) for r in cast_batch(again, batch)]
            assert got == [model.cast_one(pi, v) for pi, v in batch] and got[1][0] == 6 and got[1][3] == 0
            check_against_model(again, model, cap)
            logm = LedgerLogModel()
            logm.sync(model)
            assert again.commit_log() == (logm.root(n + 2), n + 2) and again.root_at(n) == root
            out.append((got, again.payouts(), again.commit_log()))
        finally:
            again.free()
    return out


# ---- refusals.  Every expected verdict is written down by hand: the base is ledger_log_model's (700
# entries, three blocks; double spends 20 of 10, 600 of 5, 300 of 299).

def refusal_cases(log):
    set_credited = lambda k, m, a, c, f: (k, m, a, c, 1)  # noqa: E731
    felt_p = lambda k, m, a, c, f: (k[:2] + (P,) + k[3:], m, a, c, f)  # noqa: E731
    acc_p = lambda k, m, a, c, f: (k, m, a, c[:3] + (P,), f)  # noqa: E731
    return [
        ("nullifier felt = p", _edit(log, s650=felt_p), NON_CANONICAL, "non-canonical entry \\(entry 650\\)"),
        ("account felt = p", _edit(log, s511=acc_p), NON_CANONICAL, "non-canonical entry \\(entry 511\\)"),
        ("flags = 2", _edit(log, s256=lambda k, m, a, c, f: (k, m, a, c, 2)), NON_CANONICAL,
         "non-canonical entry \\(entry 256\\)"),
        ("numbers swapped over a block edge", _swap_numbers(log, 255, 256), ORDER,
         "transfer numbers out of order \\(entry 256\\)"),
        ("a credited double spend", _edit(log, s600=set_credited), CREDIT_RULE,
         "credit rule broken \\(entry 600, its nullifier first at entry 5\\)"),
        ("a first entry left uncredited", _edit(log, s10=lambda k, m, a, c, f: (k, m, a, c, 0)), CREDIT_RULE,
         "credit rule broken \\(entry 10, its nullifier first at entry 10\\)"),
        ("two credited doubles in two blocks", _edit(log, s600=set_credited, s20=set_credited), CREDIT_RULE,
         "credit rule broken \\(entry 20, its nullifier first at entry 10\\)"),
        ("two non-canonical in two blocks", _edit(log, s650=felt_p, s3=acc_p), NON_CANONICAL,
         "non-canonical entry \\(entry 3\\)"),
        ("two swaps in two blocks", _swap_numbers(_swap_numbers(log, 610, 611), 30, 31), ORDER,
         "transfer numbers out of order \\(entry 31\\)"),
        ("order before the credit rule", _edit(_swap_numbers(log, 500, 501), s20=set_credited), ORDER,
         "transfer numbers out of order \\(entry 501\\)"),
    ]


def check_restore_refusals(ctx, ledger_factory):
    import pytest
    from ledger_log_model import BASE_N, base_log
    from qp_wormhole import QpError
    log, root, totals, payouts, _ = base_log(ledger_factory)

    def again(bad, **kw):
        led = restore(ctx, [ROOT_A], arrays_of(bad), **kw)
        try:
            return led.cast_count, led.admitted, led.credited, led.accounts, led.recount()
        finally:
            led.free()

    good = (log[-1][1] + 1, BASE_N, totals[0], len(payouts), (totals[0], BASE_N, totals[1]))
    assert again(log, root=root) == good
    for what, bad, status, text in refusal_cases(log):
        assert restore_verdict(bad, root)[0] == status, what
        with pytest.raises(ValueError, match="the log fails its audit: " + text):
            again(bad, root=root)
        assert again(log) == good, what  # a following good restore works
    # the root alone: a double spend's amount rewritten (reasons 1-3 hold); no root expected, it restores
    limb = lambda k, m, a, c, f: (k, m, (a[0], a[1], a[2], a[3] ^ 1), c, f)  # noqa: E731
    rewritten = _edit(log, s300=limb)
    assert restore_verdict(rewritten, root) == (ROOT, None, None)
    with pytest.raises(ValueError, match="the log fails its audit: claimed root differs$"):
        again(rewritten, root=root)
    assert again(rewritten) == good
    with pytest.raises(QpError, match="QP_ERR_ARG.*cast_count"):
        again(log, cast_count=log[-1][1])
    assert again(log, cast_count=log[-1][1] + 5)[0] == log[-1][1] + 5
    with pytest.raises(QpError, match="QP_ERR_ARG.*capacity"):
        again(log, capacity=BASE_N - 1)
    with pytest.raises(QpError, match="QP_ERR_ARG.*empty log has no root"):
        again([], root=root)
    assert again(log, capacity=BASE_N, root=root) == good
    # n == 0 with any cast_count: qp_ledger_new plus the counter
    empty = restore(ctx, [ROOT_A], arrays_of([]), cast_count=5, capacity=4)
    try:
        assert (empty.cast_count, empty.admitted, empty.credited, empty.accounts, empty.capacity) == (5, 0, 0, 0, 4)
        assert empty.payouts() == [] and empty.payouts_between(0, 0) == []
        res = cast_batch(empty, sized_items(2))
        assert [(r.status, r.number) for r in res] == [(0, 5), (0, 6)]
    finally:
        empty.free()
    assert again([])[:2] == (0, 0)  # cast_count=None on an empty log: 0


# ---- payout rounds

def check_round_identities(ctx, ledger_factory, name):
    """on stream `name` in batches of 7: payouts_between(0, n) == payouts(); every round between two cuts
    equals the model's, and per account the rounds add up to the cumulative total; the log-only form on
    entries() gives the same rows"""
    from qp_wormhole import ledger_log_payouts
    cap, roots, padding, items = make_stream(name)
    led = ledger_factory(roots, padding, cap)
    try:
        ns = [0]
        for kind, arg in batches(items, 7):
            if kind == "reserve":
                led.reserve(arg)
            else:
                cast_batch(led, arg)
                if led.admitted != ns[-1]:
                    ns.append(led.admitted)
        n = led.admitted
        entries, cumulative = led.entries(), led.payouts()
        log = log_of(entries)
        assert led.payouts_between(0, n) == cumulative == rows(payouts_between(log, 0, n))
        total, out = {}, []
        for m0, m1 in zip(ns, ns[1:]):
            got = led.payouts_between(m0, m1)
            assert got == rows(payouts_between(log, m0, m1)), (name, m0, m1)
            for acc, t, _ in got:
                total[acc] = total.get(acc, 0) + t
            out.append(got)
        assert total == {acc: t for acc, t, _ in cumulative}
        if n:
            m0 = ns[len(ns) // 2]
            assert ledger_log_payouts(ctx, entries, m0, n) == led.payouts_between(m0, n)
            assert ledger_log_payouts(ctx, entries) == cumulative
        return out
    finally:
        led.free()


def check_round_ranges(ctx, ledger_factory):
    """the ranges m0 in {0, 7, 255, 256, 257} x m1 in {m0, m0 + 1, 300, 513} on a 513-entry log with runs
    of double spends across the block edges; a range of double spends only; an account credited before
    m0 and again inside; the call changes nothing of the ledger"""
    import pytest
    from qp_wormhole import QpError, ledger_log_payouts
    n = 513
    led = ledger_factory([ROOT_A], None, n)
    try:
        cast_batch(led, edge_items(n))
        entries = led.entries()
        log = log_of(entries)
        nullifiers = np.ascontiguousarray(entries[0])
        before = ((led.cast_count, led.admitted, led.credited, led.accounts, led.capacity), led.payouts(),
                  led.find(nullifiers), led.commit_log())
        out = []
        for m0 in (0, 7, 255, 256, 257):
            for m1 in (m0, m0 + 1, 300, 513):
                got = led.payouts_between(m0, m1)
                assert got == rows(payouts_between(log, m0, m1)), (m0, m1)
                assert got == ledger_log_payouts(ctx, entries, m0, m1), (m0, m1)
                # no rows iff the range is empty or lies inside the run of double spends 250..262
                assert (got == []) == (m0 == m1 or (250 <= m0 and m1 <= 263)), (m0, m1)
                out.append(got)
        assert not any(e[4] for e in log[251:262]) and led.payouts_between(251, 262) == []  # double spends only
        assert ledger_log_payouts(ctx, entries, 251, 262) == []
        # five accounts in turn: the account of entry 0 is credited again at entry 5; from m0 = 1 its row
        # carries the in-range sum and first_seq 5
        assert log[0][3] == log[5][3] and log[0][4] and log[5][4]
        row = [r for r in led.payouts_between(1, 12) if r[0] == account_bytes(log[0][3])]
        assert row == [(account_bytes(log[0][3]), amount_of(log[5][2]) + amount_of(log[10][2]), 5)]
        for m0, m1 in ((2, 1), (0, n + 1), (n + 1, n + 1), (2**63, 2**63)):
            with pytest.raises(QpError, match="QP_ERR_ARG.*not a range"):
                led.payouts_between(m0, m1)
            with pytest.raises(QpError, match="QP_ERR_ARG.*not a range"):
                ledger_log_payouts(ctx, entries, m0, m1)
        assert before == ((led.cast_count, led.admitted, led.credited, led.accounts, led.capacity), led.payouts(),
                          led.find(nullifiers), led.commit_log())
        return out
    finally:
        led.free()


def check_round_big(ctx, ledger_factory, n=4096, cut=1000):
    """n entries of 2^128 - 1 to one account, split at `cut`: limb sums of cut (2^32 - 1) and (n - cut)
    (2^32 - 1) each, exact"""
    from qp_wormhole import ledger_log_payouts
    rng = np.random.default_rng(4096)
    nuls = rng.integers(0, P, size=(n, 4), dtype=np.uint64).tolist()
    led = ledger_factory([ROOT_A], None, n)
    try:
        cast_batch(led, [(transfer(k, MAX_AMOUNT, [9, 8, 7, 6]), 0) for k in nuls])
        out = []
        for m0, m1 in ((0, cut), (cut, n)):
            acc, sums, seq = led.payouts_between(m0, m1, raw=True)
            assert acc.tolist() == [[9, 8, 7, 6]] and seq.tolist() == [m0]
            assert sums.tolist() == [[(m1 - m0) * (2**32 - 1)] * 4]
            assert led.payouts_between(m0, m1) == [(account_bytes([9, 8, 7, 6]), (m1 - m0) * MAX_AMOUNT, m0)]
            out.append((acc.tolist(), sums.tolist(), seq.tolist()))
        entries = raw_entries(led)
        assert ledger_log_payouts(ctx, entries, cut, n) == led.payouts_between(cut, n)
        assert led.payouts_between(0, n) == led.payouts()
        return out
    finally:
        led.free()


def check_round_sizing(ctx, ledger_factory):
    """the C calls: the sizing call, then the filling call; cap smaller than the count stores the first
    cap rows only and the count is right; both forms"""
    from qp_wormhole._native import lib
    n = 300
    led = ledger_factory([ROOT_A], None, n)
    try:
        cast_batch(led, sized_items(n, seed=31, accounts=9))
        nul, num, amt, acc_log, fl = raw_entries(led)
        want = led.payouts_between(10, 290, raw=True)
        assert len(want[2]) == 9
        L, c = lib(), None if ctx is None else ctx.h

        def both(cap, a, s, f, count):
            p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
            assert L.qp_ledger_payouts_between(led.h, 10, 290, cap, p(a), p(s), p(f), ctypes.byref(count)) == 0
            got = (None if a is None else a.copy(), None if s is None else s.copy(), None if f is None else f.copy(),
                   count.value)
            count.value = 0
            for x in (a, s, f):
                if x is not None:
                    x[:] = 0xA5
            assert L.qp_ledger_log_payouts_between(c, acc_log.ctypes.data, amt.ctypes.data, fl.ctypes.data, n, 10, 290,
                                                   cap, p(a), p(s), p(f), ctypes.byref(count)) == 0
            assert count.value == got[3] and all(x is None or (x == y).all() for x, y in zip((a, s, f), got))
            return got

        count = ctypes.c_uint64(77)
        assert both(0, None, None, None, count)[3] == 9
        a, s, f = np.zeros((9, 4), np.uint64), np.zeros((9, 4), np.uint64), np.zeros(9, np.uint64)
        got = both(9, a, s, f, count)
        assert all((x == y).all() for x, y in zip(got[:3], want)) and got[3] == 9
        a, s, f = (np.full(x.shape, 0xA5, np.uint64) for x in (a, s, f))
        got = both(4, a, s, f, count)
        assert got[3] == 9 and all((x[:4] == y[:4]).all() and (x[4:] == 0xA5).all() for x, y in zip(got[:3], want))
        return [x.tolist() for x in want]
    finally:
        led.free()
