"""The committed walks of tests/state_walk.py, on the model alone: what they cover, and that the comparison of tests/test_gpu_state_walk.py
notices a context that breaks a rule.  No device is used: the contexts here are state_walk.FakeContext, whose answers are hashes of exactly
the state an answer may depend on (the built library is loaded all the same, for the parameter blocks the operations fill in); its kept
voxels and its voxel linearisation are tests/voxels_ref.py's own, so that the bitwise items of those probes hold on it too."""
import collections

import pytest

import state_walk as W

LIVE = ("keep", "set", "source", "window", "follow", "voxels", "robust")
# states that must meet under a probe that launches kernels, and orders of calls that must occur, each at least MEET times over all walks
MEET = 5
MEETINGS = ("voxels and window live under a launching probe", "mode 1 and kept source normals under a launching probe",
            "a robust kernel under a frames_n, frames_g or batch probe", "keep_target_voxels accepted right behind a launch under a live window")


def walk_facts(seed, ops):
    """one walk on the model and on the unplanted fake (which must pass) -> what it covers"""
    f = dict(acc=collections.Counter(), ref=collections.Counter(), pairs=set(), live=collections.Counter(), points=0, options=set(),
             crop_nothing=0, gated=collections.Counter(), ends=collections.Counter(), meet=collections.Counter(), keep_nothing=0,
             follow_update=0, bad_options=set())
    m = W.Model()
    launched = False                                        # the step before was an accepted single-pose launch of the first engine
    for name, args in ops:
        live, before = m.window_live(), (m.map, m.vm)
        rc = W.apply(m, None, (name, args))
        assert rc is not None, (seed, name, args)
        (f["acc"] if rc == W.OK else f["ref"])[name] += 1
        f["crop_nothing"] += name == "crop" and rc == W.E_INVALID and args.get("frac") == 2.0
        if name == "gated_other":
            f["gated"][args["which"]] += 1
        if name == "gate_end":
            f["ends"]["open" if args["open"] and not live else "abort"] += 1
        if name == "keep_target_voxels" and rc == W.OK:
            f["keep_nothing"] += m.vm is None
            f["meet"][MEETINGS[3]] += bool(m.vm and live and launched)
        if name == "set_option" and rc == W.E_INVALID:
            f["bad_options"].add((args["key"], args["value"]))
        # a map update that changed the map with normals_follow on while voxels were kept
        f["follow_update"] += W.CLASS[name] == "update" and rc == W.OK and m.map is not before[0] and bool(before[1]) and bool(m.opts["normals_follow"])
        launched = name in ("linearize", "icp_run") and rc == W.OK
    f["refused"] = sum(f["ref"].values())
    seen = []

    def on_check(s, kind, m, ran):
        seen.append((s, kind, ran, (bool(m.tn and m.tn[0] == "keep"), bool(m.tn and m.tn[0] == "set"), bool(m.sn), m.window_live(),
                                    bool(m.opts["normals_follow"]), bool(m.vm), m.opts["robust_kernel"] != 0),
                     tuple(k for k in W.TOGGLES if m.opts[k] != W.DEFAULTS[k])))
        if ran and kind in W.LAUNCHING:
            f["meet"][MEETINGS[0]] += bool(m.vm and m.window_live())
            f["meet"][MEETINGS[1]] += bool(m.opts["voxels_source_cov"] and m.sn)
            f["meet"][MEETINGS[2]] += bool(m.opts["robust_kernel"] and kind in ("frames_n", "frames_g", "batch"))
    W.run_walk(W.FakeContext, seed, ops, W.EVERY, on_check=on_check)
    checks = W.check_points(ops, W.EVERY)
    changing = [s for s, (n, _) in enumerate(ops) if W.CLASS[n] in W.STATE_CLASSES]
    f["gap"] = max(sum(1 for c in changing if lo < c <= hi) for lo, hi in zip([-1] + checks[:-1], checks))
    for s in sorted({r[0] for r in seen}):
        f["points"] += 1
        for key, on in zip(LIVE, next(r for r in seen if r[0] == s)[3]):
            f["live"][key] += on
    for s, kind, ran, _, off_default in seen:
        if not ran:
            continue
        before = [c for c in changing if c <= s]          # the state-changing step right before the probe: nothing in between resets it
        if before:
            f["pairs"].add((W.CLASS[ops[before[-1]][0]], kind))
        if kind not in ("map", "flags"):
            f["options"] |= set(off_default)                # an option away from its default while a probe that launches kernels ran
    return f


def conditions(facts, n_steps):
    """the names of the coverage conditions the walks miss (none: all hold)"""
    missed = []
    acc = sum((f["acc"] for f in facts), collections.Counter())
    ref = sum((f["ref"] for f in facts), collections.Counter())
    missed += ["accepted 3 times: " + n for n in sorted(W.OPS) if acc[n] < 3 and n != "gated_other"]     # (the refused call of a gate)
    missed += ["refused once: " + n for n in W.refusable() if ref[n] < 1]
    missed += ["refusals above a quarter of a walk"] * any(4 * f["refused"] > n_steps for f in facts)
    pairs = set().union(*[f["pairs"] for f in facts])
    missed += ["pair %s, %s" % (c, k) for c in W.STATE_CLASSES for k in W.PROBE_KINDS if (c, k) not in pairs]
    points = sum(f["points"] for f in facts)
    live = sum((f["live"] for f in facts), collections.Counter())
    missed += ["live at a quarter of the probe points: " + k for k in LIVE if 4 * live[k] < points]
    options = set().union(*[f["options"] for f in facts])
    missed += ["option off its default under a probe: " + k for k in W.TOGGLES if k not in options]
    missed += ["a crop that keeps nothing"] * (sum(f["crop_nothing"] for f in facts) < 1)
    gated = sum((f["gated"] for f in facts), collections.Counter())
    missed += ["refused behind a gate: " + k for k in W.GATED_OTHERS if gated[k] < 1]
    ends = sum((f["ends"] for f in facts), collections.Counter())
    missed += ["gate ended by %s twice" % k for k in ("open", "abort") if ends[k] < 2]
    meet = sum((f["meet"] for f in facts), collections.Counter())
    missed += ["%d times: %s (%d)" % (MEET, k, meet[k]) for k in MEETINGS if meet[k] < MEET]
    missed += ["a keep that keeps no voxel"] * (sum(f["keep_nothing"] for f in facts) < 1)
    missed += ["a map update with normals_follow on while voxels were kept"] * (sum(f["follow_update"] for f in facts) < 1)
    bad_options = set().union(*[f["bad_options"] for f in facts])
    missed += ["option value refused: %s = %r" % kv for kv in W.REFUSED_OPTIONS if kv not in bad_options]
    return missed


@pytest.fixture(scope="module")
def walks():
    return {seed: W.walk_ops(seed, W.N_STEPS) for seed in W.SEEDS}


@pytest.fixture(scope="module")
def facts(walks):
    return [walk_facts(seed, ops) for seed, ops in walks.items()]


def test_the_generator_is_deterministic(walks):
    for seed, ops in walks.items():
        assert len(ops) == W.N_STEPS
        assert repr(W.walk_ops(seed, W.N_STEPS)) == repr(ops)
        assert eval(repr(ops)) == ops                    # a walk prints as a literal that replay accepts
    assert len({repr(ops) for ops in walks.values()}) == len(W.SEEDS)


def test_every_operation_with_a_refusal_is_in_the_list_the_walks_must_refuse():
    """an operation whose own prediction can be a refusal - on an empty context, on a full one, or through its refused form - is refusable"""
    rng = W.np.random.default_rng(0)
    full = W.replay(None, [("keyframes_reset", {}), ("keyframes_add", {}), ("places_reset", {}), ("set_target", {}), ("set_source", {})])
    only_store = W.replay(None, [("keyframes_reset", {}), ("keyframes_add", {}), ("places_reset", {})])
    found = set()
    for name in W.OPS:
        for m in (W.Model(), only_store, full):
            for form in W._draw_args(rng, name, m):
                if form is not None and W.apply(W.clone(m), None, (name, form)) not in (None, W.OK):
                    found.add(name)
    assert sorted(found - {"gated_other"}) == sorted(set(W.refusable()) - {"gated_other"})


def test_the_committed_walks_cover_what_they_must(facts):
    acc = sum((f["acc"] for f in facts), collections.Counter())
    ref = sum((f["ref"] for f in facts), collections.Counter())
    print("operation:accepted/refused " + " ".join("%s:%d/%d" % (n, acc[n], ref[n]) for n in sorted(W.OPS)))
    print("probe points %d, live %r, most state-changing steps between two checks %d" %
          (sum(f["points"] for f in facts), dict(sum((f["live"] for f in facts), collections.Counter())), max(f["gap"] for f in facts)))
    print("meetings %r, keeps that keep nothing %d, followed updates under kept voxels %d" %
          (dict(sum((f["meet"] for f in facts), collections.Counter())), sum(f["keep_nothing"] for f in facts), sum(f["follow_update"] for f in facts)))
    assert conditions(facts, W.N_STEPS) == []


@pytest.mark.parametrize("fault", W.FAULTS)
def test_a_planted_fault_is_caught(walks, fault):
    caught = []
    for seed, ops in walks.items():
        try:
            W.run_walk(lambda: W.FakeContext(fault), seed, ops, W.EVERY, make_fresh=W.FakeContext)
        except (AssertionError, W.Unexpected) as e:      # (a probe that differs, or a return code the model did not expect)
            caught.append(seed)
            assert "seed %r, step" % seed in str(e) and "replay(ctx, [" in str(e)
    assert caught, fault
