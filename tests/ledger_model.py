"""The transfer ledger's semantics as a model (a dict from nullifier to transfer
number, a dict of account totals as exact ints, and the screening order), named
transfer streams, and run_stream, which casts a stream into a ledger and checks
every result, the state, the log, find, the payouts, the totals and the recount
against the model.  Shared by the host-path and the device-path tests; the model
is the oracle for both.

Home-slot rule the crafted streams rely on (csrc/ledger_table.h): a ledger of
capacity C has S = the power of two >= 2 C slots in each of its two tables; a
nullifier's home slot is nullifier[0] & (S - 1), an account's is
exit_account[0] & (S - 1); the probe goes to the next slot, wrapping."""
import random

import numpy as np

P = 0xFFFFFFFF00000001
ROOT_A = [11, 12, 13, P - 1]
ROOT_B = [21, 22, 23, 24]
ROOT_UNKNOWN = [11, 12, 13, P - 2]
MAX_AMOUNT = 2**128 - 1

CREDITED, PROOF_REJECTED, MALFORMED, PADDING, BAD_AMOUNT, UNKNOWN_ROOT, DOUBLE_SPEND = range(7)
BATCHINGS = [1, 7, 64, None]  # None: every run of transfers between two reserves as one batch


def limbs_of(amount):
    return [(amount >> (96 - 32 * i)) & 0xFFFFFFFF for i in range(4)]


def transfer(nullifier, amount=1, account=(1, 2, 3, 4), root=ROOT_A, limbs=None):
    return list(nullifier) + list(root) + (limbs_of(amount) if limbs is None else list(limbs)) + list(account)


class Model:
    def __init__(self, roots, padding=None):
        self.roots, self.padding = [list(r) for r in roots], None if padding is None else list(padding)
        self.seen, self.seq_of, self.log, self.cast = {}, {}, [], 0
        self.totals, self.first_seq, self.order = {}, {}, []

    def screen(self, pi, verdict):
        if verdict:
            return PROOF_REJECTED
        if len(pi) != 16 or any(not 0 <= x < P for x in pi):
            return MALFORMED
        if self.padding is not None and list(pi) == self.padding:
            return PADDING
        if any(x >> 32 for x in pi[8:12]):
            return BAD_AMOUNT
        if list(pi[4:8]) not in self.roots:
            return UNKNOWN_ROOT
        return CREDITED

    def cast_one(self, pi, verdict):
        """(status, verify_status, number, first)"""
        num, self.cast = self.cast, self.cast + 1
        st = self.screen(pi, verdict)
        if st:
            return (st, verdict, num, num)
        nul, acc = tuple(pi[0:4]), tuple(pi[12:16])
        amount = sum(x << (96 - 32 * i) for i, x in enumerate(pi[8:12]))
        first = self.seen.setdefault(nul, num)
        seq = len(self.log)
        self.log.append((nul, num, amount, acc, first == num))
        if first != num:
            return (DOUBLE_SPEND, verdict, num, first)
        self.seq_of[nul] = seq
        if acc not in self.totals:
            self.order.append(acc)
            self.first_seq[acc] = seq
        self.totals[acc] = self.totals.get(acc, 0) + amount
        return (CREDITED, verdict, num, num)

    def payouts(self):
        return [(acc, self.totals[acc], self.first_seq[acc]) for acc in self.order]


def _keys(rng, n):
    return [[rng.randrange(P) for _ in range(4)] for _ in range(n)]


def _homed(rng, home, slots):
    """a felt 0 whose home slot in a table of `slots` slots is `home`"""
    return (rng.randrange(1, 1 << 40) * slots) | home


REJECTS = [lambda n: (transfer(n), 5),                                  # a rejected proof
           lambda n: (transfer(n[:3] + [P]), 0),                        # malformed
           lambda n: (transfer(n, limbs=[0, 1 << 32, 0, 0]), 0),        # bad amount
           lambda n: (transfer(n, root=ROOT_UNKNOWN), 0)]               # unknown root


def _runs(rng, n, run, only_last=False):
    """n transfers whose admitted and rejected ones alternate in runs of `run` (the first run is
    rejected); only_last: all rejected but the last.  A tenth of the admitted ones are double spends."""
    nuls, accounts, items = _keys(rng, n), _keys(rng, 5), []
    for i in range(n):
        admitted = (i == n - 1) if only_last else (i // run) % 2 == 1
        if admitted:
            nul = nuls[i] if i < 10 or i % 10 else nuls[i - 2 * run]
            items.append((transfer(nul, rng.randrange(MAX_AMOUNT + 1), accounts[i % 5]), 0))
        else:
            items.append(REJECTS[(i // 2) % 4](nuls[i]))
    return items


def make_stream(name):
    """(capacity, roots, padding, items): an item is (public inputs, verdict) or ("reserve", capacity)"""
    rng = random.Random("ledger " + name)
    amount = lambda: rng.randrange(MAX_AMOUNT + 1)  # noqa: E731
    roots, padding = [ROOT_A], None
    if name == "distinct":
        acc = _keys(rng, 5)
        cap, items = 32, [(transfer(n, amount(), acc[i % 5]), 0) for i, n in enumerate(_keys(rng, 32))]
    elif name == "one_nullifier":
        n, acc = _keys(rng, 1)[0], _keys(rng, 3)
        cap, items = 64, [(transfer(n, amount(), acc[i % 3]), 0) for i in range(64)]
    elif name == "across_batches":
        acc = _keys(rng, 4)
        first = [(transfer(n, amount(), acc[i % 4]), 0) for i, n in enumerate(_keys(rng, 32))]
        cap, items = 64, first + [(transfer(pi[0:4], amount(), acc[(i + 1) % 4]), 0) for i, (pi, _) in enumerate(first)]
    elif name == "screened":
        roots = [ROOT_A, ROOT_B]
        g = _keys(rng, 8)
        padding = transfer(g[7], 77, [9, 9, 9, 9])
        acc = [5, 6, 7, 8]
        cap, items = 16, [
            (transfer(g[0], 10, acc), 0),
            (transfer(g[1], 10, acc), 4),                                   # a rejected proof, all else fine
            (transfer(g[1][:3] + [P], 10, acc), 0),                         # a felt of exactly p
            (list(padding), 0),                                             # the padding inputs
            (transfer(g[1], 10, acc, limbs=[0, 0, 1 << 32, 5]), 0),         # a limb of exactly 2^32
            (transfer(g[1], 10, acc, root=ROOT_UNKNOWN), 0),                # unknown root: g[1] stays unspent
            (transfer(g[1], 11, acc, root=ROOT_B), 0),                      # ... and is credited under an accepted one
            (transfer(g[1], 12, acc), 0),                                   # a double under another accepted root
            (transfer(g[2], 10, acc, root=ROOT_UNKNOWN, limbs=[1 << 32, 0, 0, 0]), 0),  # two failures: the amount's first
            (transfer(g[2][:3] + [P], 10, acc, root=ROOT_UNKNOWN), 9),      # rejected proof before anything else
            (transfer(g[2], 10, acc, limbs=[P, 0, 0, 0]), 0),               # malformed before bad amount
            (list(padding)[:15] + [8], 0),                                  # one felt off the padding: a transfer
            (transfer(g[0], 99, [1, 1, 1, 1]), 0),                          # a double of the first transfer
            (transfer(g[3], 10, acc)[:15], 0),                              # 15 public inputs
            (transfer(g[3], 0, acc), 0),                                    # an amount of 0
            (transfer(g[4], MAX_AMOUNT, acc, limbs=[0xFFFFFFFF] * 4), 0),   # every limb at its maximum
        ]
    elif name in ("padding_known", "padding_unknown"):
        pad = transfer(_keys(rng, 1)[0], 1000, _keys(rng, 1)[0])
        padding = pad if name == "padding_known" else None
        other = (transfer(_keys(rng, 1)[0], 5, [4, 4, 4, 4]), 0)
        cap, items = 16, [(list(pad), 0)] * 4 + [other] + [(list(pad), 0)] * 4
    elif name == "big_amounts":
        acc, other = _keys(rng, 2)
        items = [(transfer(n, MAX_AMOUNT, acc), 0) for n in _keys(rng, 513)]
        items += [(transfer(n, 0, other), 0) for n in _keys(rng, 3)] + [(transfer(_keys(rng, 1)[0], MAX_AMOUNT, other), 0)]
        cap = 520
    elif name == "collide_nullifiers":
        # capacity 4, 8 slots: a and b share home slot 7 (b wraps to slot 0), c has a's felt 0 and another
        # felt 3 (slot 1), then b again (found through the wrapped chain); exactly full, reserve to 8 (16 slots)
        a, b = [_homed(rng, 7, 16), 1, 2, 3], [_homed(rng, 7, 16), 1, 2, 3]
        c, d = a[:3] + [4], [_homed(rng, 15, 16), 6, 6, 6]
        acc = _keys(rng, 2)
        t = lambda n, i: (transfer(n, amount(), acc[i % 2]), 0)  # noqa: E731
        cap, items = 4, [t(a, 0), t(b, 1), t(c, 2), t(b, 3), ("reserve", 8), t(c, 4), t(d, 5), t(a, 6), t(d, 7)]
    elif name == "collide_accounts":
        # the same shapes in the account table: distinct nullifiers, accounts a, b, c as above
        a, b = [_homed(rng, 7, 16), 1, 2, 3], [_homed(rng, 7, 16), 1, 2, 3]
        c, d = a[:3] + [4], [_homed(rng, 15, 16), 6, 6, 6]
        n = _keys(rng, 8)
        cap, items = 4, ([(transfer(n[i], amount(), x), 0) for i, x in enumerate((a, b, c, b))] + [("reserve", 8)] +
                         [(transfer(n[4 + i], amount(), x), 0) for i, x in enumerate((c, d, a, d))])
    elif name == "many_blocks":
        acc = _keys(rng, 64)
        order = _keys(rng, 2048) * 3
        rng.shuffle(order)
        cap, items = 8192, [(transfer(n, amount(), acc[rng.randrange(64)]), 0) for n in order]
    elif name == "rejected_only":
        cap, items = 1, [REJECTS[i % 4](n) for i, n in enumerate(_keys(rng, 9))]
    elif name == "grow":
        g, acc = _keys(rng, 100), _keys(rng, 7)
        b = lambda i: (transfer(g[i], amount(), acc[i % 7]), 0)  # noqa: E731
        items = ([b(i) for i in range(24)] + [b(3), b(3)] + [("reserve", 26), ("reserve", 64)] +
                 [b(i) for i in (0, 23, 24, 25, 5)] + [b(i) for i in range(26, 50)] + [("reserve", 128)] +
                 [b(i) for i in (1, 24, 49, 50)] + [b(i) for i in range(51, 100)] + [b(99), b(0)])
        cap = 32
    elif name.startswith("runs_"):
        _, n, run = name.split("_")
        cap, items = 1024, _runs(rng, int(n), int(run) if run != "last" else 1, only_last=run == "last")
    else:
        raise KeyError(name)
    return cap, roots, padding, items


STREAMS = ["distinct", "one_nullifier", "across_batches", "screened", "padding_known", "padding_unknown", "big_amounts",
           "collide_nullifiers", "collide_accounts", "many_blocks", "rejected_only", "grow"]
# one batch each: the stable pack across block boundaries, with blocks holding 0, some and 256 admitted
RUN_STREAMS = [f"runs_{n}_{r}" for n in (255, 256, 257, 513) for r in (1, 3, 64)] + ["runs_513_last"]


def batches(items, batching):
    """the stream as ("cast", [items]) and ("reserve", capacity) steps"""
    run = []
    for it in list(items) + [("reserve", None)]:
        if it[0] == "reserve":
            step = batching or max(len(run), 1)
            for at in range(0, len(run), step):
                yield "cast", run[at:at + step]
            run = []
            if it[1] is not None:
                yield it
        else:
            run.append(it)


def cast_batch(ledger, batch):
    rows = [pi for pi, _ in batch]
    verdicts = [v for _, v in batch]
    pis = np.array(rows, dtype=np.uint64) if all(len(r) == 16 for r in rows) else rows
    return ledger.cast_public(pis, verdicts if any(verdicts) else None, reserve=False)


def account_bytes(acc):
    return b"".join(int(x).to_bytes(8, "little") for x in acc)


def lookups(ledger, model):
    """what a reserve must not change: find of every nullifier, the payouts, every account's total"""
    return (ledger.find([list(n) for n in model.seen]) if model.seen else [], ledger.payouts(),
            ledger.totals_for([list(a) for a in model.order]) if model.order else [])


def check_against_model(ledger, model, cap):
    assert (ledger.cast_count, ledger.admitted, ledger.credited, ledger.accounts, ledger.capacity) == \
        (model.cast, len(model.log), len(model.seq_of), len(model.order), cap)
    nul, num, amt, acc, credited = ledger.entries()
    assert [tuple(int(x) for x in r) for r in nul] == [e[0] for e in model.log]
    assert [int(x) for x in num] == [e[1] for e in model.log]
    assert amt == [e[2] for e in model.log]
    assert [tuple(int(x) for x in r) for r in acc] == [e[3] for e in model.log]
    assert [bool(x) for x in credited] == [e[4] for e in model.log]
    if len(model.log) > 3:  # a window of the log
        n2, m2, a2, c2, f2 = ledger.entries(1, 2)
        assert (n2 == nul[1:3]).all() and (m2 == num[1:3]).all() and a2 == amt[1:3] and (c2 == acc[1:3]).all()
    # find: the credited entry of every nullifier ever admitted; a rejected-only or unseen one is not there
    seen = list(model.seen)
    assert ledger.find([list(n) for n in seen] + [[1, 2, 3, 5]]) == [model.seq_of[n] for n in seen] + [None]
    want = model.payouts()
    assert ledger.payouts() == [(account_bytes(a), t, s) for a, t, s in want]
    assert ledger.totals_for([list(a) for a, _, _ in want] + [[3, 1, 4, 1]]) == [t for _, t, _ in want] + [None]
    if want:
        assert ledger.total_for(account_bytes(want[-1][0])) == want[-1][1]
    assert ledger.recount() == (len(model.seq_of), len(model.log), sum(t for _, t, _ in want))


def run_stream(ledger_factory, name, batching):
    """Casts stream `name` cut into batches of `batching` into ledger_factory(roots,
    padding, capacity), checks everything observable against the model and
    returns the results (tuples), for comparison across batchings and paths."""
    cap, roots, padding, items = make_stream(name)
    model = Model(roots, padding)
    ledger = ledger_factory(roots, padding, cap)
    results = []
    try:
        for kind, arg in batches(items, batching):
            if kind == "reserve":
                before = lookups(ledger, model)
                ledger.reserve(arg)
                cap = arg
                assert lookups(ledger, model) == before
                check_against_model(ledger, model, cap)
                continue
            got = [tuple(r) for r in cast_batch(ledger, arg)]
            want = [model.cast_one(pi, v) for pi, v in arg]
            assert got == want, (name, batching, len(results))
            results += got
        check_against_model(ledger, model, cap)
    finally:
        ledger.free()
    return results
