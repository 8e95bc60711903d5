"""The weighted learn and the annealed prioritized sample on the device
(include/sacenv_weighted_learn.h).

* **Ones**: weights of 1.0 are the unweighted learn bit for bit -- weights buffer, losses and the
  whole scratch -- over three learns, for one agent and for a population of three.
* **Halves**: on fresh agents weights of 0.5 halve the critics' first moments and losses and
  quarter their second moments, bit for bit (a power of two commutes with every fp32 rounding);
  actor, value and the raw per-row squared TD errors do not move. B = 256 and B = 512.
* **A zero weight silences a row**: rewards of 0 or 1e6 on rows of weight 0 give the same critics.
* **f64 parity** against tests/weighted_sac_oracle.py: every critic gradient element within
  ``c_w 2^-24 S_max``, exactly 0 where S == 0, the critic losses in the same unit, with
  c_w = 40.3 = 4 x c_ref_w, c_ref_w = 10.08 being what torch CPU float32 shows on the same inputs
  (tests/test_weighted_learn_cpu.py, profiles/weighted_learn_f64_margins.json). Native worst on an
  MI355X: d11_m1_b256 2.72, d14_m05_b768 5.98 (the profile's ``native`` half, written with
  SACENV_WEIGHTED_RECORD=<file>).
* **Members**: each of three members with its own weight vector is a stand-alone ``NativeSAC``
  given that vector.
* **The pipeline**: ``NativeSACPopulation(importance_weights=True)`` on a prioritized replay is the
  hand-driven sample -> learn(weights=last_weights) -> update_from_learn, and the priorities follow
  the raw TD errors.
* **Annealing**: the weights at sample k are (min leaf / leaf)^beta_at(k) to 1 ulp, host-numbered
  and device-counted alike; the draw is the plain sample's.
* **The example** with ``--importance-weights --beta-final 1 --beta-anneal 8``.
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import prio_oracle
import sac_f64_cases as K
import weighted_sac_oracle as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

D = 11
_RECORD: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("SACENV_WEIGHTED_RECORD")
    if path and _RECORD:
        with open(path, "w") as f:
            json.dump(_RECORD, f, indent=1, sort_keys=True)


def _cfg(m, B, max_size=1 << 14):
    from sacenv.agent import AgentConfig
    return AgentConfig(lr_alpha=0.0015 + 0.001 * m, lr_beta=0.0003 * (m + 2), gamma=0.95 + 0.004 * m,
                       tau=0.002 * (m + 1), reward_scale=2.0 + m, batch_size=B, max_size=max_size)


def _solo(gpu, m, B):
    from sacenv.sac_native import NativeSAC
    a = NativeSAC(gpu, _cfg(m, B), obs_dim=D, init_seed=10 + m, with_memory=False)
    a.scratch.zero_()
    return a


def _pop(gpu, P, B, **kw):
    from sacenv.population import NativeSACPopulation
    kw.setdefault("with_memory", False)
    max_size = kw.pop("max_size", 1 << 14)
    p = NativeSACPopulation(gpu, [_cfg(m, B, max_size) for m in range(P)], obs_dim=D,
                            init_seeds=[10 + m for m in range(P)], **kw)
    p.scratch.zero_()
    return p


def _batch(gpu, B, seed):
    s, a, r, s2, e1, e2 = K.candidate_pool(D, B, seed)
    batch = (s, a, r, s2, K.done_pattern(B, seed))
    return tuple(t.to(gpu) for t in batch), (e1.to(gpu), e2.to(gpu))


def _stacked(gpu, P, B, seed):
    per = [_batch(gpu, B, 1000 * seed + m) for m in range(P)]
    return (per, tuple(torch.stack([per[m][0][k] for m in range(P)]) for k in range(5)),
            tuple(torch.stack([per[m][1][k] for m in range(P)]) for k in range(2)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lc_rows(agent):
    """(o1, o2): float offsets of F_LC1 / F_LC2 in one agent's learn scratch."""
    from sacenv import _lib
    o1, o2 = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().sacenv_replay_prio_learn_rows(agent._pp, C.byref(o1), C.byref(o2)))
    return o1.value, o2.value


# ---------------------------------------------------------------- 1. ones

def test_ones_are_the_unweighted_learn_one_agent(gpu, built_lib):
    B = 256
    a, b = _solo(gpu, 1, B), _solo(gpu, 1, B)
    for k in range(3):
        batch, noise = _batch(gpu, B, 50 + k)
        la = a.learn(batch, noise)
        lb = b.learn(batch, noise, weights=torch.ones(B, device=gpu))
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb)), f"learn {k}: losses"
        assert torch.equal(_bits(a.weights), _bits(b.weights)), f"learn {k}: weights buffer"
        assert torch.equal(_bits(a.scratch), _bits(b.scratch)), f"learn {k}: scratch"
    assert a.adam_step == b.adam_step == 3 and b._learn_weighted is not None and a._learn_weighted is None


def test_ones_are_the_unweighted_learn_population(gpu, built_lib):
    P, B = 3, 256
    a, b = _pop(gpu, P, B), _pop(gpu, P, B)
    for k in range(3):
        _, batch, noise = _stacked(gpu, P, B, 60 + k)
        la = a.learn(batch, noise)
        lb = b.learn(batch, noise, weights=torch.ones(P, B, device=gpu))
        torch.cuda.synchronize()
        assert torch.equal(_bits(la), _bits(lb)), f"learn {k}: losses"
        assert torch.equal(_bits(a.weights), _bits(b.weights)), f"learn {k}: weights buffer"
        assert torch.equal(_bits(a.scratch), _bits(b.scratch)), f"learn {k}: scratch"


# ---------------------------------------------------------------- 2. halves

@pytest.mark.parametrize("B", [256, 512])
def test_halves_scale_the_critics_by_powers_of_two(gpu, built_lib, B):
    a, b = _solo(gpu, 2, B), _solo(gpu, 2, B)
    batch, noise = _batch(gpu, B, 70 + B)
    la = a.learn(batch, noise)
    lb = b.learn(batch, noise, weights=torch.full((B,), 0.5, device=gpu))
    torch.cuda.synchronize()
    tiny = 2.0 ** -100
    for n in ("critic_1", "critic_2"):
        ma, mb = a.adam_state(n), b.adam_state(n)
        for k in ma["exp_avg"]:
            m0, v0 = ma["exp_avg"][k], ma["exp_avg_sq"][k]
            # no unweighted non-zero element is near the underflow range: it cannot excuse a miss
            assert float(m0[m0 != 0].abs().min()) >= tiny and float(v0[v0 != 0].min()) >= tiny, (n, k)
            assert int((m0 != 0).sum()) > 0
            assert torch.equal(_bits(mb["exp_avg"][k]), _bits(0.5 * m0)), (n, k, "exp_avg")
            assert torch.equal(_bits(mb["exp_avg_sq"][k]), _bits(0.25 * v0)), (n, k, "exp_avg_sq")
    assert torch.equal(_bits(lb[2]), _bits(0.5 * la[2])) and torch.equal(_bits(lb[3]), _bits(0.5 * la[3]))
    assert float(la[2]) > 0 and float(la[3]) > 0
    assert torch.equal(_bits(lb[0]), _bits(la[0])) and torch.equal(_bits(lb[1]), _bits(la[1]))
    for n in ("actor", "value", "target_value"):
        for (k, p), (_, q) in zip(getattr(a, n).state_dict().items(), getattr(b, n).state_dict().items()):
            assert torch.equal(_bits(p), _bits(q)), (n, k)
        if n != "target_value":
            for which in ("exp_avg", "exp_avg_sq"):
                for k, m0 in a.adam_state(n)[which].items():
                    assert torch.equal(_bits(m0), _bits(b.adam_state(n)[which][k])), (n, which, k)
    o1, o2 = _lc_rows(a)
    assert o2 == o1 + B
    raw_a, raw_b = a.scratch[o1: o1 + 2 * B], b.scratch[o1: o1 + 2 * B]
    assert torch.equal(_bits(raw_a), _bits(raw_b)) and float(raw_a.min()) >= 0 and float(raw_a.max()) > 0
    # the raw rows are the unweighted loss's terms
    assert float(la[2]) == pytest.approx(0.5 * float(raw_a[:B].double().mean()), rel=1e-5)


# ---------------------------------------------------------------- 3. a zero weight silences a row

def test_zero_weight_silences_a_row(gpu, built_lib):
    B = 256
    rows = [0, 17, B - 1]                           # first block, second block, last
    batch, noise = _batch(gpu, B, 90)
    w = torch.ones(B, device=gpu)
    w[rows] = 0.0
    runs = {}
    for reward, weights in ((0.0, w), (1e6, w), (0.0, None), (1e6, None)):
        r = batch[2].clone()
        r[rows] = reward
        ag = _solo(gpu, 0, B)
        losses = ag.learn((batch[0], batch[1], r, batch[3], batch[4]), noise, weights=weights)
        torch.cuda.synchronize()
        o1, _ = _lc_rows(ag)
        crit = [t for n in ("critic_1", "critic_2") for t in getattr(ag, n).state_dict().values()]
        crit += [t for n in ("critic_1", "critic_2") for which in ("exp_avg", "exp_avg_sq")
                 for t in ag.adam_state(n)[which].values()]
        runs[(reward, weights is not None)] = (torch.cat([t.reshape(-1) for t in crit]).clone(),
                                               torch.stack(losses[2:]).clone(), ag.scratch[o1: o1 + 2 * B].clone())
    (pa, la, ra), (pb, lb, rb) = runs[(0.0, True)], runs[(1e6, True)]
    assert torch.equal(_bits(pa), _bits(pb)), "critic parameters / moments see a row of weight 0"
    assert torch.equal(_bits(la), _bits(lb)), "critic losses see a row of weight 0"
    differ = (ra != rb).view(2, B)
    want = torch.zeros(B, dtype=torch.bool, device=gpu)
    want[rows] = True
    assert torch.equal(differ[0], want) and torch.equal(differ[1], want)       # the raw rows: exactly those rows
    for reward in (0.0, 1e6):
        p1, l1, r1 = runs[(reward, False)]
        p0, l0, r0 = runs[(reward, True)]
        assert not torch.equal(p1, p0) and not torch.equal(l1, l0)             # weight 1 on those rows is another run
        assert torch.equal(_bits(r1), _bits(r0))                                # with the same raw rows


# ---------------------------------------------------------------- 4. f64 parity

@pytest.mark.parametrize("name", ["d11_m1_b256", "d14_m05_b768"])
def test_weighted_critic_gradients_per_element(gpu, built_lib, name):
    from sacenv.sac_native import NativeSAC
    case = K.CASES[name]
    mk = lambda: NativeSAC(gpu, K.agent_config(case), obs_dim=case["obs_dim"], max_action=case["max_action"],  # noqa: E731
                           init_seed=case["seed"], with_memory=False)
    nat, plain = mk(), mk()
    sd = K.cpu_state_dicts(nat)
    batch, noise, shares = K.step_batch(sd, case, 1)
    w = W.case_weights(case)
    f = W.learn_f64_weighted(sd, batch, noise, w, K.case_cfg(case), case["max_action"])
    gb, gn = tuple(t.to(gpu) for t in batch), tuple(t.to(gpu) for t in noise)
    zeros = {n: {k: np.zeros(tuple(v.shape), np.float32) for k, v in nat.adam_state(n)["exp_avg"].items()}
             for n in K.OPTIMISED}
    losses = [float(x) for x in nat.learn(gb, gn, weights=w.to(gpu))]
    plain.learn(gb, gn)
    torch.cuda.synchronize()
    m = K.np_state({n: nat.adam_state(n)["exp_avg"] for n in K.OPTIMISED})
    g = {n: {k: K.grad_from_moments(v) for k, v in m[n].items()} for n in K.OPTIMISED}
    units, _ = K.grad_units(g, f)
    units.update(K.loss_units(losses, f))
    crit = W.critic_units(units)
    dead = sum(int((S == 0).sum()) for n in W.WEIGHTED for S in f["S"][n].values())
    dead_bad = K.dead_nonzero_from_moments(m, zeros, f)
    print(f"{name}: rejected {shares['kink']:.3f} weights [{float(w.min()):.4f}, {float(w.max())}] "
          f"worst {max(crit.values()):.2f} of {W.C_W} units {crit}")
    _RECORD[name] = {"rejected_share": shares["kink"], "worst": max(crit.values()), "units": crit,
                     "dead_elements": dead, "dead_nonzero": dead_bad}
    assert shares["kink"] <= K.MAX_REJECT
    assert len(crit) == 14
    assert dead > 0 and dead_bad == 0, "a gradient element whose every contribution is 0 is not exactly 0"
    bad = {k: v for k, v in crit.items() if not v <= W.C_W}
    assert not bad, (name, bad)
    for n in ("actor", "value"):          # untouched by the weights: the unweighted run's, bit for bit
        for k, v in nat.adam_state(n)["exp_avg"].items():
            assert torch.equal(_bits(v), _bits(plain.adam_state(n)["exp_avg"][k])), (n, k)
    for n in W.WEIGHTED:
        assert not torch.equal(nat.adam_state(n)["exp_avg"]["fc2.weight"], plain.adam_state(n)["exp_avg"]["fc2.weight"])


# ---------------------------------------------------------------- 5. members

def test_members_take_their_own_weights(gpu, built_lib):
    P, B = 3, 256
    per, batch, noise = _stacked(gpu, P, B, 7)
    ws = torch.stack([W.draw_weights(B, 300 + m) for m in range(P)]).to(gpu)
    assert not torch.equal(ws[0], ws[1]) and not torch.equal(ws[1], ws[2])
    pop = _pop(gpu, P, B)
    lp = pop.learn(batch, noise, weights=ws)
    solos = [_solo(gpu, m, B) for m in range(P)]
    ls = [solos[m].learn(per[m][0], per[m][1], weights=ws[m]) for m in range(P)]
    torch.cuda.synchronize()
    for m in range(P):
        assert torch.equal(_bits(pop.weights[m]), _bits(solos[m].weights)), f"member {m}: slab"
        assert torch.equal(_bits(lp[m]), _bits(torch.stack(ls[m]))), f"member {m}: losses"
    # a member given ones is its unweighted run, whatever the others get
    mixed = ws.clone()
    mixed[1] = 1.0
    pop2 = _pop(gpu, P, B)
    lq = pop2.learn(batch, noise, weights=mixed)
    plain = _solo(gpu, 1, B)
    l1 = plain.learn(per[1][0], per[1][1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(pop2.weights[1]), _bits(plain.weights)) and torch.equal(_bits(lq[1]), _bits(torch.stack(l1)))
    for m in (0, 2):
        assert torch.equal(_bits(pop2.weights[m]), _bits(pop.weights[m]))
    assert not torch.equal(pop2.weights[1], pop.weights[1])
    with pytest.raises(ValueError, match="weights must be"):
        pop.learn(batch, noise, weights=ws[0])
    assert pop.adam_step == 1


# ---------------------------------------------------------------- 6. the pipeline

def _rows(P, n, g):
    return (torch.rand((P, n, D), generator=g), torch.rand((P, n, 1), generator=g) * 2 - 1,
            torch.rand((P, n), generator=g), torch.rand((P, n, D), generator=g),
            (torch.rand((P, n), generator=g) < 0.1).to(torch.uint8))


def test_pipeline_is_the_hand_driven_sequence(gpu, built_lib):
    from sacenv.prioritized import PrioritizedPopulationReplay
    from sacenv.sac_native import _SacCore
    P, B, M, n = 3, 256, 1024, 96
    seeds = [1000 + 7 * m for m in range(P)]
    reps = [PrioritizedPopulationReplay(P, M, (D,), 1, device=gpu, seeds=list(range(P)), prio_seeds=seeds)
            for _ in range(3)]
    kw = dict(max_size=M, noise_seeds=[100, 101, 102])
    auto = _pop(gpu, P, B, replay=reps[0], importance_weights=True, **kw)
    hand = _pop(gpu, P, B, replay=reps[1], **kw)          # driven by hand below: its own learn() is not called
    off = _pop(gpu, P, B, replay=reps[2], **kw)           # importance_weights=False
    assert auto.importance_weights and not hand.importance_weights
    g = torch.Generator().manual_seed(4)
    o1, _ = _lc_rows(auto)
    stride = int(auto.pop_layout.scratch_bytes) // 4
    learns, w_min = 0, 1.0
    for it in range(20):
        rows = _rows(P, n, g)
        for r in reps:
            r.store_batch(*rows)
        before = [reps[0].levels(m)[0] for m in range(P)]
        hdr = [reps[0].header(m) for m in range(P)]
        la = auto.learn()
        lc = off.learn()
        lb = None
        if reps[1].mem_cntr >= B:
            b5 = reps[1].sample(B, as_bool=False)[:5]
            lb = _SacCore.learn(hand, b5, weights=reps[1].last_weights)
            reps[1].update_from_learn(hand)
        assert (la is None) == (lb is None) == (lc is None)
        if la is None:
            continue
        learns += 1
        torch.cuda.synchronize()
        assert torch.equal(_bits(la), _bits(lb)), f"iteration {it}: losses"
        assert torch.equal(auto.weights.view(torch.int32), hand.weights.view(torch.int32)), f"iteration {it}: weights"
        assert torch.equal(reps[0].prio, reps[1].prio), f"iteration {it}: a tree level"
        assert torch.equal(reps[0].last_weights, reps[1].last_weights)
        w_min = min(w_min, float(reps[0].last_weights.min()))     # (the first sample's leaves are all max_leaf)
        # the priorities follow the RAW scratch rows
        idx, scratch = reps[0].last_idx.cpu().numpy(), auto.scratch.cpu().numpy()
        for m in range(P):
            t = prio_oracle.Tree(M)
            t.leaf, t.max_leaf = [int(v) for v in before[m]], hdr[m]["max_leaf"]
            a, b = scratch[m * stride + o1:][:B], scratch[m * stride + o1 + B:][:B]
            t.update_td(idx[m], a, b, reps[0].alpha, reps[0].eps)
            lv = reps[0].levels(m)
            assert np.array_equal(lv[0][idx[m]], np.array(t.leaf, np.uint32)[idx[m]]), f"iteration {it} member {m}: leaves"
            t.leaf = [int(v) for v in lv[0]]
            for k_, (have, want) in enumerate(zip(lv, t.levels())):
                assert [int(v) for v in have] == want, f"iteration {it} member {m}: level {k_}"
    torch.cuda.synchronize()
    assert learns == 18 and auto.adam_step == hand.adam_step == off.adam_step == learns
    assert torch.equal(reps[0].arena, reps[1].arena) and torch.equal(reps[0].arena, reps[2].arena)
    assert w_min < 0.5 and not torch.equal(auto.weights, off.weights)       # weights below 1 were applied
    assert reps[0].sample_calls == reps[1].sample_calls == learns


# ---------------------------------------------------------------- 7. annealing

def test_annealed_weights(gpu, built_lib):
    from sacenv.prioritized import PrioritizedPopulationReplay
    P, B, M, N = 3, 256, 1024, 6
    seeds = [1000 + 7 * m for m in range(P)]

    def new(**kw):
        return PrioritizedPopulationReplay(P, M, (D,), 1, device=gpu, seeds=list(range(P)), prio_seeds=seeds,
                                           beta=0.4, **kw)
    host, dev_, plain, dplain, flat = (new(beta_final=1.0, beta_anneal=N), new(beta_final=1.0, beta_anneal=N), new(),
                                       new(), new(beta_final=0.4, beta_anneal=N))
    all_ = (host, dev_, plain, dplain, flat)
    g = torch.Generator().manual_seed(12)
    rng = np.random.default_rng(12)
    rows = _rows(P, 700, g)
    idx, leaf = rng.integers(0, 700, (P, 400)), rng.integers(1, 1 << 22, (P, 400))
    for r in all_:
        r.store_batch(*rows)
        r.set_priorities(idx, leaf)
    assert host.beta_at(0) == 0.4 and host.beta_at(N) == 1.0 and flat.beta_at(3) == 0.4
    for k in range(10):
        outs = [r.sample(B, as_bool=False, graph_safe=r in (dev_, dplain)) for r in all_]
        torch.cuda.synchronize()
        assert dev_.header(1)["calls"] == dplain.header(1)["calls"] == k + 1 and host.header(1)["calls"] == 0
        assert host.sample_calls == k + 1 and dev_.sample_calls == 0
        for r, o in zip(all_[1:], outs[1:]):               # the draw is the plain sample's
            assert torch.equal(r.last_idx, host.last_idx) and torch.equal(r.last_leaf, host.last_leaf), k
            for u, v in zip(o[:5], outs[0][:5]):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        assert torch.equal(_bits(host.last_weights), _bits(dev_.last_weights)), f"sample {k}: host and device numbering"
        assert torch.equal(_bits(plain.last_weights), _bits(dplain.last_weights))
        assert torch.equal(_bits(flat.last_weights), _bits(plain.last_weights)), f"sample {k}: beta_final == beta"
        if k in (0, 3, N, 9):
            lf = host.last_leaf.cpu().numpy().view(np.uint32)
            got = host.last_weights.cpu().numpy()
            for m in range(P):
                want = prio_oracle.weights(lf[m], host.beta_at(k))
                assert prio_oracle.ulp_distance_f32(got[m], want).max() <= 1, (k, m)
                assert len(set(lf[m].tolist())) > 8
            if k == 0:
                assert torch.equal(_bits(host.last_weights), _bits(plain.last_weights))
            else:
                assert not torch.equal(host.last_weights, plain.last_weights)
    assert host.beta_at(9) == 1.0


# ---------------------------------------------------------------- 8. the example

def test_the_example_runs_with_importance_weights(gpu, built_lib, capsys):
    spec = importlib.util.spec_from_file_location("train_population",
                                                  os.path.join(ROOT, "examples", "train_population.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--members", "2", "--envs-per-member", "64", "--batch", "256", "--iters", "12", "--prioritized"]
    torch.manual_seed(1234)
    plain = mod.main(base)
    torch.manual_seed(1234)
    out = mod.main(base + ["--importance-weights", "--beta-final", "1", "--beta-anneal", "8"])
    torch.manual_seed(1234)
    fixed = mod.main(base + ["--importance-weights", "0.5"])
    capsys.readouterr()
    new = ("importance_weights", "beta_final", "beta_anneal", "beta_now")
    assert not any(k in plain["prioritized"] for k in new) and plain["prioritized"]["beta"] == 0.4
    pr = out["prioritized"]
    assert pr["importance_weights"] is True and pr["beta"] == 0.4 and pr["beta_final"] == 1.0
    assert pr["beta_anneal"] == 8 and pr["beta_now"] == 1.0
    assert fixed["prioritized"]["beta"] == 0.5 and fixed["prioritized"]["beta_final"] is None
    assert fixed["prioritized"]["beta_now"] == 0.5 and fixed["prioritized"]["importance_weights"] is True
    assert out["losses"] is not None and np.isfinite(np.array(out["losses"])).all()
    assert out["losses"] != plain["losses"]
    for bad in (["--replay", "members", "--importance-weights"], ["--importance-weights", "-1"],
                ["--importance-weights", "--beta-final", "1"], ["--beta-final", "1", "--beta-anneal", "8"],
                ["--importance-weights", "--beta-final", "1", "--beta-anneal", "0"]):
        with pytest.raises(SystemExit):
            mod.main(base + bad)
    with pytest.raises(SystemExit):
        mod.main(base[:-1] + ["--importance-weights"])          # without --prioritized
    capsys.readouterr()
