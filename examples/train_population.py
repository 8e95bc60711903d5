"""A hyper-parameter search on one GPU: P SAC agents, each on its own N boat envs.

main.py -p (main.py:215-235) for P agents at once. The reference draws each agent's actor and
critic learning rates, gamma and tau (utils/hyperparameter_tuner.py:20-43) and trains the agents
as OS processes, three at a time; here they are the members of one ``NativeSACPopulation``:

* one ``VecBoatEnv`` of P x N envs; member m owns envs [m N, (m + 1) N);
* per step: one act launch for all members, one env step, one store launch and one sample (two
  launches) for all members through a ``PopulationReplay``, one learn (four launches) for all
  members; ``--replay members`` keeps one ``DeviceReplayBuffer`` per member instead (a store, a
  draw and a gather launch per member and five stack copies per step): the same table and
  losses, bit for bit;
* an ``EpisodeLog`` on the env; an episode of env e belongs to member e // N.

    python examples/train_population.py --members 4 --envs-per-member 1024 --iters 200 [--seed 0]
        [--replay population|members] [--share-replay K] [--prioritized [ALPHA] [--importance-weights [BETA]
        [--beta-final B1 --beta-anneal N]]] [--noise torch|counter] [--noise-seed 0] [--keep-best DIR]
        [--select-every K [--quantile Q] [--min-episodes E] [--select-seed 0]] [--keep-traces DIR
        [--render DIR [--render-every K]]]

``--share-replay K`` (with ``--replay population``) pools the members' experience: K of the
``--batch`` rows every member learns from are drawn from all members' buffers, the other rows from
its own (``PopulationReplay.sample(pool_rows=K)``, include/sacenv_population_share.h: still two
launches per sample). A stored row is the env's own (obs, action, reward, obs', terminal), so it is
valid data for every member; a member starts to learn once its own buffer holds a batch, as
before. With K > 0 a member's run depends on the other members' rows, so it is no longer the run
that member makes alone. The JSON line gains ``pool_rows``; with 0 the run is the one without the
flag, and without the flag nothing changes.

``--prioritized [ALPHA]`` (with ``--replay population``, without ``--share-replay``) replays the
surprising transitions more often: the replay is a ``PrioritizedPopulationReplay``
(include/sacenv_prioritized_replay.h), every member samples its own rows in proportion to (|TD error|
+ eps)^ALPHA (default 0.6) from a sum tree on the device, new rows enter at the largest priority so
far, and after each learn the batch's rows take the priorities of the TD errors the learn kernels
left behind. The importance weights (``replay.last_weights``) are applied in the learn with
``--importance-weights`` (below) and not without it; whether prioritizing speeds learning up has not
been measured, with or without them. The JSON line gains ``prioritized`` (alpha, beta, eps and each
member's priority total). Without the flag nothing changes.

``--importance-weights [BETA]`` (with ``--prioritized``) applies the sample's importance weights,
(min leaf / leaf)^BETA (default 0.4), to the critics' TD loss (``NativeSACPopulation(...,
importance_weights=True)``, include/sacenv_weighted_learn.h): each batch row's critic gradient and
loss term is scaled by its weight, while the priorities still follow the raw TD errors.
``--beta-final B1 --beta-anneal N`` let the exponent run from BETA to B1 over the first N samples,
computed on the device from the sample's number. ``prioritized`` in the JSON line gains
``importance_weights``, ``beta_final``, ``beta_anneal`` and ``beta_now`` (the last sample's exponent).
Without the flag nothing changes.

``--noise counter`` gives member m the noise seed ``--noise-seed`` + m (``sacenv.PolicyNoise``): the
act draw and both learn draws of an iteration come from one launch for all members, and member m's
run is the run a stand-alone ``NativeSAC(noise_seed=...)`` on envs [m N, (m + 1) N) makes, bit for
bit, whatever P is. ``--noise torch`` (the default) draws from torch's device stream.

Prints the members' drawn values (the four numbers a tuned_configs.yaml differs in, one line per
member), then what main.py:99-114 prints per model -- Score (the last finished episode), Best
Score, Average over the look-back -- and one JSON line with the same. ``--save DIR`` writes every
member's checkpoints to DIR/member_<m>/checkpoints/: the members' LAST weights.

``--keep-best DIR`` keeps what the reference would have on disk instead: it saves a model whenever
an episode's score beats the look-back average (main.py:106-108). A ``MemberScoreboard`` follows
the episode log on the device, is updated after every ``learn`` and snapshots the weights of the
members the rule selects; at the end its table is printed beside the post-hoc one, and the
snapshots go to DIR/member_<m>/checkpoints/ with DIR/overview.csv (main.py:121-128).

``--select-every K`` turns the search into population-based training: every K iterations a
``PopulationSelection`` ranks the members by their look-back mean on the device and the worst
``--quantile`` of those that finished ``--min-episodes`` episodes since their last replacement
become copies of the best -- weights, Adam moments and all -- with the winner's four values, each
times 0.8 or 1.2 and clipped to the search ranges. One line is printed per replacement, and the
JSON line gains ``selection`` (per member: rank, times replaced, parent, current values) and
``replacements``. The table's drawn values are then the members' LAST ones. Without the flag
nothing changes.

``--keep-traces DIR`` keeps the episodes the reference would render: a ``BestEpisodes`` holds the
recent steps of every env on the device and, whenever an episode ends with a score above its
member's best, keeps its rows (one ``update`` per iteration, two launches). At the end its table is
printed, each member's best episode goes to DIR/member_<m>/episodes/episode_0_data.csv in the
reference's format, and the JSON line gains ``traces``. Without the flag nothing changes.

``--render DIR [--render-every K]`` (with ``--keep-traces``) draws those episodes as main.py -r does:
at the end an ``EpisodeFrames`` draws every K-th step of each member's best episode on the device
-- the track, the path so far, the boat at its heading, the action and rudder strip with a cursor --
and writes DIR/member_<m>/rendering/episode_0.gif; one line is printed and the JSON line gains
``frames`` (per member the frame count and the file). Without the flag nothing changes.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sac-agent_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--envs-per-member", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0, help="seed of the hyper-parameter draws")
    ap.add_argument("--lookback", type=int, default=100, help="avg_lookback (main.py:100-101)")
    ap.add_argument("--save", default=None, help="directory for the members' checkpoints")
    ap.add_argument("--replay", choices=("population", "members"), default="population",
                    help="one PopulationReplay for all members, or one DeviceReplayBuffer per member")
    ap.add_argument("--share-replay", type=int, default=None, metavar="K",
                    help="K of every member's batch rows are drawn from all members' buffers (0: its own only; "
                         "needs --replay population)")
    ap.add_argument("--prioritized", type=float, nargs="?", const=0.6, default=None, metavar="ALPHA",
                    help="sample every member's rows in proportion to (|TD error| + eps)^ALPHA (needs --replay "
                         "population; excludes --share-replay)")
    ap.add_argument("--importance-weights", type=float, nargs="?", const=0.4, default=None, metavar="BETA",
                    help="apply the sample's importance weights (min leaf / leaf)^BETA in the critic loss (needs "
                         "--prioritized; bare: 0.4)")
    ap.add_argument("--beta-final", type=float, default=None, metavar="B1",
                    help="anneal the weights' exponent from BETA to B1 (needs --importance-weights and --beta-anneal)")
    ap.add_argument("--beta-anneal", type=int, default=None, metavar="N",
                    help="the samples the exponent takes from BETA to B1")
    ap.add_argument("--noise", choices=("torch", "counter"), default="torch",
                    help="policy noise from torch's stream, or counter-based with one seed per member")
    ap.add_argument("--noise-seed", type=int, default=0, help="member m's noise seed is this + m")
    ap.add_argument("--keep-best", default=None, metavar="DIR",
                    help="snapshot a member whenever an episode of its beats the look-back average; write the "
                         "snapshots and overview.csv to DIR")
    ap.add_argument("--select-every", type=int, default=0, metavar="K",
                    help="every K iterations the worst members copy the best (0: never)")
    ap.add_argument("--quantile", type=int, default=None,
                    help="how many members lose, and how many may be copied from (default: members // 4)")
    ap.add_argument("--min-episodes", type=int, default=None,
                    help="episodes a member finishes after a replacement before it is ranked again "
                         "(default: --lookback)")
    ap.add_argument("--select-seed", type=int, default=0, help="seed of the selection's draws")
    ap.add_argument("--keep-traces", default=None, metavar="DIR",
                    help="keep each member's best episode step by step on the device; write them to DIR as the "
                         "reference's episode CSVs")
    ap.add_argument("--render", default=None, metavar="DIR",
                    help="draw each member's best episode on the device and write it to DIR as a GIF (needs "
                         "--keep-traces)")
    ap.add_argument("--render-every", type=int, default=1, metavar="K", help="draw every K-th step and the last")
    ap.add_argument("--max-episode-steps", type=int, default=500)
    args = ap.parse_args(argv)
    if args.render and not args.keep_traces:
        ap.error("--render draws the episodes --keep-traces keeps")
    share = args.share_replay or 0
    if not 0 <= share <= args.batch:
        ap.error("--share-replay takes 0 to --batch rows")
    if share and args.replay != "population":
        ap.error("--share-replay draws from the one arena of --replay population")
    if args.prioritized is not None:
        if args.replay != "population":
            ap.error("--prioritized keeps its priorities beside the one arena of --replay population")
        if args.share_replay is not None:
            ap.error("--prioritized samples a member's own rows: it excludes --share-replay")
        if not 0 <= args.prioritized < float("inf"):
            ap.error("--prioritized takes a finite ALPHA >= 0")
    if args.importance_weights is not None:
        if args.prioritized is None:
            ap.error("--importance-weights applies the weights of a --prioritized sample")
        if not 0 <= args.importance_weights < float("inf"):
            ap.error("--importance-weights takes a finite BETA >= 0")
    if args.beta_final is not None or args.beta_anneal is not None:
        if args.importance_weights is None:
            ap.error("--beta-final and --beta-anneal anneal the exponent of --importance-weights")
        if args.beta_final is None or args.beta_anneal is None:
            ap.error("--beta-final and --beta-anneal go together")
        if not 0 <= args.beta_final < float("inf") or args.beta_anneal < 1:
            ap.error("--beta-final takes a finite B1 >= 0, --beta-anneal N >= 1")
    P, N = args.members, args.envs_per_member
    if N < 64 or N % 64:
        raise SystemExit("--envs-per-member must be a multiple of 64 (the act kernel's row block)")
    from sacenv import NativeSACPopulation, PopulationReplay, VecBoatEnv, sample_hpsets
    from sacenv.agent import AgentConfig
    from sacenv.episodes import EpisodeLog
    dev = torch.device("cuda")
    configs = sample_hpsets(P, args.seed, base=AgentConfig(batch_size=args.batch))
    pooled = args.replay == "population"
    replay = None
    weighted = args.importance_weights is not None
    if args.prioritized is not None:
        from sacenv import PrioritizedPopulationReplay
        extra = {}
        if weighted:
            extra.update(beta=args.importance_weights)
            if args.beta_final is not None:
                extra.update(beta_final=args.beta_final, beta_anneal=args.beta_anneal)
        replay = PrioritizedPopulationReplay(P, configs[0].max_size, (11,), 1, device=dev, seeds=list(range(P)),
                                             alpha=args.prioritized, **extra)
    elif pooled:  # the members' buffers in one arena, with the seeds the per-member buffers get
        replay = PopulationReplay(P, configs[0].max_size, (11,), 1, device=dev, seeds=list(range(P)))
    pop = NativeSACPopulation(dev, configs, init_seeds=list(range(P)), buffer_seeds=list(range(P)), replay=replay,
                              pool_rows=share, **({"importance_weights": True} if weighted else {}),
                              noise_seeds=[args.noise_seed + m for m in range(P)] if args.noise == "counter" else None)
    for m, mem in enumerate(pop.members):
        print(f"member {m}: " + json.dumps(mem.hpset()))
    env = VecBoatEnv({"base_settings": {"experiment": 6, "test_mode": 0}}, P * N, seed=0, device=dev,
                     max_episode_steps=args.max_episode_steps)
    obs = env.reset().clone()
    log = EpisodeLog(env)
    board = selection = scores = None
    if args.keep_best:
        from sacenv import MemberScoreboard
        board = MemberScoreboard(log, P, N, lookback=args.lookback, population=pop)
    if args.select_every > 0:
        from sacenv import MemberScoreboard, PopulationSelection
        # the look-back means the selection ranks by: --keep-best's board, or one without a snapshot
        scores = board if board is not None else MemberScoreboard(log, P, N, lookback=args.lookback)
        selection = PopulationSelection(scores, pop, quantile=args.quantile, min_episodes=args.min_episodes,
                                        seed=args.select_seed)
    traces = None
    if args.keep_traces:
        from sacenv import BestEpisodes
        traces = BestEpisodes(env, members=P, envs_per_member=N)
    replacements = []
    # terminal as main.py:83-88 stores it: each env's last termination, kept per member
    last_term = [torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(P)]
    losses = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        eps = noise = None
        if pop.noise is not None:  # the act draw and both learn draws of this iteration: one launch
            eps, noise = pop.noise_for_step(N)
        a = pop.choose_action(obs.view(P, N, -1), eps=eps)
        env.step(a.view(-1))
        log.update()
        if traces is not None:
            traces.update(a.view(-1))
        if pooled:  # member m's rows are envs [m N, (m + 1) N): the env's outputs as they lie
            replay.store_env_step(obs, a, env)
        for m in range(0 if pooled else P):
            rows = slice(m * N, (m + 1) * N)
            pop.remember(m, obs[rows], a[m], env.reward[rows], env.obs[rows], env.term[rows],
                         final_state=env.final_obs[rows], last_term=last_term[m])
        obs = env.obs.clone()
        out = pop.learn(noise=noise, losses=False)
        losses = out if out is not None else losses
        if board is not None:  # after learn: where main.py:106 saves
            board.update()
        if selection is not None and it % args.select_every == args.select_every - 1:
            if scores is not board:
                scores.update()
            for r in selection.step():  # two launches, then the one read-back: the new values go to learn's table
                replacements.append({"iter": it, **r})
                print(f"iter {it}: member {r['member']} <- member {r['source']}: "
                      + json.dumps(pop.members[r["member"]].hpset()))
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    entries = log.drain()  # (the board reads what is left first)
    owner = entries["env"] // N
    table = []
    fmt = lambda x: f"{x:12.2f}" if x is not None else f"{'-':>12}"  # noqa: E731
    print(f"{'member':>6} {'episodes':>8} {'Score':>12} {'Best Score':>12} {'Average':>12}")
    for m in range(P):
        scores = entries["score"][owner == m]
        row = {"member": m, "episodes": int(scores.size), **pop.members[m].hpset(),
               "score": float(scores[-1]) if scores.size else None,
               "best_score": float(scores.max()) if scores.size else None,
               "avg_score": float(np.mean(scores[-args.lookback:])) if scores.size else None}
        if board is not None:  # the save rule post hoc, as main.py:99-108 words it
            ends, history, saves, last_save = entries["end_step"][owner == m], [], 0, None
            for score, end in zip(scores.tolist(), ends.tolist()):
                history.append(score)
                if score > np.mean(history[-args.lookback:]):
                    saves, last_save = saves + 1, end
            row.update(saves=saves, last_save_step=last_save)
        table.append(row)
        print(f"{m:>6} {row['episodes']:>8} {fmt(row['score'])} {fmt(row['best_score'])} {fmt(row['avg_score'])}")
    if args.save:
        pop.save_models(args.save, optimizer=True)
    device_table = kept = None
    if board is not None:
        device_table = board.table()
        print("on the device:")
        print(f"{'member':>6} {'episodes':>8} {'Score':>12} {'Best Score':>12} {'Average':>12} {'saves':>6} "
              f"{'last save':>10}")
        for row in device_table:
            print(f"{row['member']:>6} {row['episodes']:>8} {fmt(row['score'])} {fmt(row['best_score'])} "
                  f"{fmt(row['avg_score'])} {row['saves']:>6} {str(row['last_save_step']):>10}")
        kept = board.save_models(args.keep_best)
        print(f"best member {board.best_member()}; snapshots of members {kept} in {args.keep_best}")
    trace_table = None
    if traces is not None:
        trace_table = traces.table()
        print("best episodes:")
        print(f"{'member':>6} {'Score':>12} {'env':>8} {'end step':>10} {'length':>7} {'rows':>6} {'replaced':>8}  ending")
        for row in trace_table:
            print(f"{row['member']:>6} {fmt(row['score'])} {str(row['env']):>8} {str(row['end_step']):>10} "
                  f"{row['length']:>7} {row['rows']:>6} {row['replaced']:>8}  {row['term'] or '-'}")
        written = traces.save_csv(args.keep_traces)
        print(f"best episodes of members {written} in {args.keep_traces}")
    frame_table = None
    if args.render:
        from sacenv import EpisodeFrames
        frames = EpisodeFrames(traces, every=args.render_every)
        drawn = frames.save_gif(args.render)
        frame_table = [{"member": m, "frames": len(frames.frame_steps(m)),
                        "file": os.path.join(args.render, f"member_{m}", "rendering", "episode_0.gif")
                        if m in drawn else None} for m in range(P)]
        print(f"frames of members {drawn} in {args.render}")
    out = {"pipeline": "population act + VecBoatEnv.step + " + ("population store + population sample" if pooled else
                                                                  "per-member store + per-member sample")
                       + " + population learn", "replay": args.replay, "noise": args.noise,
           "members": P, "envs_per_member": N, "iters": args.iters, "batch": args.batch,
           "env_steps_per_s": P * N * args.iters / el, "ms_per_iter": el / args.iters * 1e3,
           "losses": None if losses is None else losses.tolist(), "table": table}
    if args.share_replay is not None:
        out.update(pool_rows=share)
    if args.prioritized is not None:
        out.update(prioritized={"alpha": replay.alpha, "beta": replay.beta, "eps": replay.eps,
                                "totals": [replay.total(m) for m in range(P)]})
        if weighted:
            out["prioritized"].update(importance_weights=True, beta_final=replay.beta_final,
                                      beta_anneal=replay.beta_anneal,
                                      beta_now=replay.beta_at(max(replay.sample_calls - 1, 0)))
    if board is not None:
        out.update(device_table=device_table, kept=kept, best_member=board.best_member())
    if selection is not None:
        out.update(selection=selection.table(), replacements=replacements)
    if traces is not None:
        out.update(traces=trace_table)
    if frame_table is not None:
        out.update(frames=frame_table)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
