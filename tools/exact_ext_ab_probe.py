#!/usr/bin/env python3
"""The exact extended and per-runout entries (mcq_exact_ext_kernel, mcq_exact_runout_kernel) and the four hero-range
entries, whose kernels share their block prologue, of this build beside the parent commit's build and a second copy of it:
the loop and the rule of tools/ab_common.py.

    timeout -k 10 900 python tools/exact_ext_ab_probe.py PARENT_SO COPY_SO [ONLY]
                                      ONLY: the shapes whose name contains it, e.g. "kind 1"

Shapes, one per kernel body at least, chosen so that an owner walks many completions, each under both laws:
    kind 0 (a lane per completion)    AhAd against known KsKc before the flop: plain, split-pot and per-seat rows
    kind 1 (a wave per completion)    AhKh + known QsQc against one top-25 % opponent, before the flop and on a flop (the
                                      records of tools/exact_seats_probe.py): plain, split-pot and per-seat rows
    kind 2 (a block per completion)   9c8c against two opponents with any hand on a flop
    per runout                        169 flop records (tools/runout_probe.py), hero against known AsAd (kind 0) and
                                      against one opponent with any hand (kind 1)
    hero range                        all four entries on one flop shape and one preflop shape
The rounds per shape come from the parent's call time (CALL_BUDGET_MS of calls per library and order, MIN_ROUNDS at
least).  Exit status 1 if a shape is slower than its interval; one that is faster is printed as such."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ab_common  # noqa: E402
import hero_preflop_weighted_probe as hero  # noqa: E402
import runout_probe  # noqa: E402

PASSES = 4
CALL_BUDGET_MS, MIN_ROUNDS, MAX_ROUNDS = 150.0, 3, 100
HERO_SHAPES = [("flop, top 25% vs top 25%", ["2D", "9H", "JS"], 0.25, 0.25, 0),
               ("preflop, {AA, AKs} vs top 10%", [], {"AA", "AKS"}, 0.10, 0)]
# entry -> number of output arrays after the law
ENTRIES = {"ext": 2, "ext_ways": 2, "seats": 1, "ext_seats": 1, "ext_runouts": 2}


class Lib(hero.Baseline):
    """... and the exact extended entries of that build."""

    def __init__(self, path):
        super().__init__(path)
        vp = C.c_void_p
        for entry, n_out in ENTRIES.items():
            getattr(self.lib, "mcq_exact_batch_" + entry).argtypes = [vp, vp, vp, C.c_size_t, C.c_int] + [vp] * n_out

    def ext(self, entry, q, x, law, outs):
        rc = getattr(self.lib, "mcq_exact_batch_" + entry)(self.ctx, q.ctypes.data, x.ctypes.data, len(q), law,
                                                           *[o.ctypes.data for o in outs])
        assert rc == 0, (entry, rc)
        return outs


def ext_cases():
    import neuron_poker_amd as npa
    from neuron_poker_amd import _lib
    from neuron_poker_amd.montecarlo_hip import _opponent_range_bits
    ids = lambda cs: [npa.card_id(c) for c in cs]  # noqa: E731
    top25 = _opponent_range_bits(0.25)
    rows = {"ext": (_lib.EXACT_PROB_DTYPE, _lib.RESULT_DTYPE), "ext_ways": (_lib.EXACT_PROB_WAYS_DTYPE, _lib.RESULT_WAYS_DTYPE),
            "seats": (_lib.RESULT_SEATS_DTYPE,), "ext_seats": (_lib.RESULT_SEATS_DTYPE,)}
    shapes = []  # name, entries, q, x
    q = _lib.pack_query_one(ids(["AH", "AD"]), [], 2, 1)
    shapes.append(("kind 0, AhAd vs KsKc preflop", ("ext", "ext_ways", "seats"), q, _lib.pack_query_ext(1, known=[ids(["KS", "KC"])])))
    for name, board in (("preflop", []), ("flop 2c7d9h", ["2C", "7D", "9H"])):
        q = _lib.pack_query_one(ids(["AH", "KH"]), ids(board), 3, 1)
        x = _lib.pack_query_ext(1, known=[ids(["QS", "QC"])], opp_range=top25)
        shapes.append(("kind 1, AhKh + QsQc vs top 25%, " + name, ("ext", "ext_ways", "ext_seats"), q, x))
    q = _lib.pack_query_one(ids(["9C", "8C"]), ids(["7C", "6D", "2S"]), 3, 1)
    shapes.append(("kind 2, 9c8c vs 2 x any, flop 7c6d2s", ("ext",), q, _lib.pack_query_ext(1)))
    cases = []
    for name, entries, q, x in shapes:
        for entry in entries:
            outs = [[np.zeros(len(q), dt) for dt in rows[entry]] for _ in range(3)]
            for law in (0, 1):
                cases.append(((entry, name + (", reference law" if law == 0 else "")),
                              lambda b, slot, entry=entry, q=q, x=x, law=law, outs=outs: b.ext(entry, q, x, law, outs[slot])))
    table = ids(runout_probe.FLOP)
    heroes = [h for h in runout_probe.class_hands(table + ids(["AS", "AD"]))]
    flops = np.concatenate([_lib.pack_query_one(h, table, 2, 1) for h in heroes])
    for name, x in (("kind 0, 169 flops vs AsAd", _lib.pack_query_ext(len(heroes), known=[ids(["AS", "AD"])])),
                    ("kind 1, 169 flops vs any", _lib.pack_query_ext(len(heroes)))):
        outs = [[np.zeros((len(heroes), _lib.RUNOUT_CARD_ROWS), _lib.RESULT_WAYS_DTYPE),
                 np.zeros((len(heroes), _lib.HAND_ROWS), _lib.RESULT_WAYS_DTYPE)] for _ in range(3)]
        for law in (0, 1):
            cases.append((("ext_runouts", name + (", reference law" if law == 0 else "")),
                          lambda b, slot, x=x, law=law, outs=outs: b.ext("ext_runouts", flops, x, law, outs[slot])))
    return cases


def main(parent_so, copy_so, only=""):
    from neuron_poker_amd import _lib
    _lib.load_library()
    cases = ext_cases() + [(key, call) for key, _, call in hero.ab_cases(HERO_SHAPES)]
    cases = [c for c in cases if only in c[0][1]]
    parent = Lib(parent_so)                                            # the rounds per shape, from the parent's call time
    timed = []
    for key, call in cases:
        call(parent, 1)
        t0 = time.perf_counter()
        call(parent, 1)
        ms = (time.perf_counter() - t0) * 1e3
        timed.append((key, max(MIN_ROUNDS, min(MAX_ROUNDS, int(CALL_BUDGET_MS / ms))), call))
        print("%-28s %-52s parent %9.3f ms -> %3d rounds per order" % (key[0], key[1], ms, timed[-1][1]), flush=True)
    parent.close()
    return ab_common.ab(Lib, (_lib.library_path(), parent_so, copy_so), timed, PASSES, faster_fails=False)


if __name__ == "__main__":
    sys.exit(0 if main(*sys.argv[1:4]) else 1)
