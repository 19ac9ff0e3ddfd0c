"""CPU-only: the model of k_keep's sign map (tests/keep_signs_cases.py) over the two sweeps.

1. The existing steady-state sweep (tests/test_gpu_steady_fuzz.py) requires, after a poison event,
   all of level S+2 to be the oracle's.  The rule may therefore skip nothing in a build that
   follows one: over its default seed the model must find no skipped row segment there (its
   images flip sign between consecutive builds).  A later change to the rule, or to that sweep's
   draw, that breaks this fails here, without a GPU.
2. The sign-map sweep's default seed reaches every path of the rule at least five times.
"""
import collections

import keep_signs_cases as ks
import numpy as np
import steady_cases as sc


def test_the_existing_sweep_never_skips_after_a_poison_event():
    mode2 = after_poison = 0
    for case in sc.cases(sc.DEFAULT_SEED, sc.DEFAULT_CASES):
        for rec in ks.walk(case, sc.images(case)):
            if rec["mode"] != 2:
                continue
            mode2 += 1
            if rec["poisoned"]:
                after_poison += 1
                skipped = int((~rec["stored"]).sum())
                assert skipped == 0, (f"{skipped} row segments skipped after a poison event: the existing sweep's store "
                                      f"map would keep the poison in level S+2", rec["k"], rec["span"], case)
    # the sweep does reach the rule (else this test checks nothing)
    assert mode2 >= 10 and after_poison >= 3, (mode2, after_poison)


def _coverage(cases):
    n = collections.Counter()
    for case in cases:
        imgs = ks.images(case)
        for rec in ks.walk(case, imgs):
            st = case["builds"][rec["k"]]
            if rec["mode"] == 1:
                n["establish after: " + rec["after"]] += 1
            if rec["mode"] != 2:
                continue
            stored, old, neg = rec["stored"], rec["old"], rec["neg"]
            skipped = int((~stored).sum())
            n["mode 2 builds"] += 1
            n["skipped segments"] += skipped
            n["builds with a skip"] += skipped > 0
            n["builds re-storing because of old"] += bool((old & ~neg).any())
            n["builds re-storing because of new"] += bool((neg & ~old).any())
            if skipped:
                n["skip on a band"] += case["bands"] is not None
                n["skip on batch > 1"] += case["B"] > 1
                n["skip with a bound input"] += bool(st["in_bound"])
                n["skip after a poison event"] += rec["poisoned"]
                n["skip with keep_kernel %d" % st["keep_kernel"]] += 1
    return n


def test_default_seed_reaches_every_path_of_the_rule():
    n = _coverage(ks.cases(ks.DEFAULT_SEED, ks.DEFAULT_CASES))
    print(dict(n))
    need = ["builds with a skip", "builds re-storing because of old", "builds re-storing because of new", "skip on a band",
            "skip on batch > 1", "skip with a bound input", "skip after a poison event", "skip with keep_kernel 1",
            "skip with keep_kernel 2"] + ["establish after: " + w for w in ks.INVALIDATIONS]
    short = {k: n[k] for k in need if n[k] < 5}
    assert not short, (short, dict(n))


def test_the_draw_is_pure_and_the_images_are_what_the_rule_needs():
    a, b = ks.cases(ks.DEFAULT_SEED, 12), ks.cases(ks.DEFAULT_SEED, 12)
    assert a == b and all(len(c["builds"]) == ks.N_BUILDS and len(c["events"]) == ks.N_BUILDS - 1 for c in a)
    for case in a:
        x, y = ks.images(case), ks.images(case)
        for k, st in enumerate(case["builds"]):
            for p, q in zip(x[k], y[k]):
                assert np.array_equal(p, q) and p.shape == (case["H"], case["W"])
                assert p.dtype == (np.uint8 if st["fmt"] == "u8" else np.int32)


def test_the_model_of_one_context():
    m = ks.SignMap(20, 260, 1)
    st = dict(k_keep=True, fmt="i32")
    img = np.ones((20, 260), np.int32)
    assert m.build(dict(k_keep=False, fmt="i32"), [img])[0] == 0 and not m.known
    mode, stored, neg = m.build(st, [img])
    assert mode == 1 and stored.all() and not neg.any() and m.known and stored.shape == (1, 20, 2)
    neg_img = img.copy()
    neg_img[7, 259] = -1
    mode, stored, neg = m.build(st, [neg_img])
    assert mode == 2 and stored.sum() == 1 and stored[0, 7, 1]
    mode, stored, neg = m.build(st, [img])  # restores +0 over the -0
    assert mode == 2 and stored.sum() == 1 and stored[0, 7, 1] and not m.flags.any()
    mode, stored, neg = m.build(st, [img])
    assert mode == 2 and not stored.any()
    assert m.build(dict(k_keep=True, fmt="u8"), [img.astype(np.uint8)])[0] == 0 and not m.known
    assert m.build(st, [img])[0] == 1
