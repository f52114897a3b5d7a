"""Measure the pure-MCTS parameter sweep (onitama_az.parameter_check) on one GPU and write
profiles/parameter_check_<date>.json.

The n sweep at the reference's size (36 pairings x 100 games, 1 600 playouts, clock off), three ways in one
process:
  lockstep    ParameterCheck.play(): all pairings' games in one launch per ply;
  sequential  ParameterCheck.play(sequential=True): pairing after pairing, one launch per pairing and ply;
  fights      36 x evaluator.fight(Mcts_i, Mcts_k): what the sweep cost before per-root parameters (two launches
              per ply, on two threads; other rollout streams, so only its time compares).
The ways run in rounds of alternating order (--ways chooses them, --rounds how often each); lockstep and
sequential must report identical results. Then one oaz_pure_mcts_search_each call against one
oaz_pure_mcts_search call with the same uniform parameters at G = 1, 64 and 3 600: what per-root parameters cost.
Every leg's figures are printed as they come and the file is rewritten after every leg.
"""
import argparse
import datetime
import json
import socket
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "onitama-alphazero_amd"))

from onitama_az.evaluator import EvaluatorConfig, fight  # noqa: E402
from onitama_az.game import Deck, initial_state_np  # noqa: E402
from onitama_az.parameter_check import N_VALUES, ParameterCheck, pairings  # noqa: E402
from onitama_az.pure_mcts import Mcts, pure_mcts_search, pure_mcts_search_each  # noqa: E402


def run_way(way, a):
    """One pass over the whole sweep: (seconds, plies, launches, results or None)."""
    t0 = time.perf_counter()
    if way in ("lockstep", "sequential"):
        pc = ParameterCheck("n", N_VALUES, game_amnt=a.game_amnt, max_playouts=a.playouts, seed=a.seed,
                            verbose=way == "sequential")  # (a line per pairing as it ends: the leg takes minutes)
        res = pc.play(sequential=way == "sequential")
        dt = time.perf_counter() - t0
        return dt, sum(sum(r.plies) for r in res), pc.launches, [(r.results, r.plies) for r in res]
    plies = launches = 0
    for i, k in pairings(N_VALUES):
        agents = [Mcts(search_time=0.4, min_node_visits=n, exploration_c=1.0, max_playouts=a.playouts, seed=a.seed)
                  for n in (N_VALUES[i], N_VALUES[k])]
        st = fight(EvaluatorConfig(game_amnt=a.game_amnt, max_plies=150, seed=a.seed), *agents)
        plies += sum(st.plies)
        launches += agents[0]._calls + agents[1]._calls
        print(f"  fights: n = {N_VALUES[i]} vs {N_VALUES[k]} done, {time.perf_counter() - t0:.1f} s", flush=True)
    return time.perf_counter() - t0, plies, launches, None


def summary(legs):
    t = [x["seconds"] for x in legs]
    rate = [x["plies"] / x["seconds"] for x in legs]
    return {"rounds": len(legs), "seconds_median": statistics.median(t), "seconds_range": [min(t), max(t)],
            "plies_per_s_median": statistics.median(rate), "plies_per_s_range": [min(rate), max(rate)],
            "plies": legs[0]["plies"], "launches": legs[0]["launches"]}


def per_root_cost(a, reps=3):
    G_all = a.game_amnt * len(pairings(N_VALUES))
    roots = np.concatenate([initial_state_np(Deck.default(a.seed, q).indices()) for q in range(G_all)])
    out = []
    for G in sorted({1, 64, G_all}):
        r = np.ascontiguousarray(roots[:G])
        ways = {"search": lambda: pure_mcts_search(r, a.playouts, 1, 1.0, seed=a.seed, game_id0=0),
                "search_each": lambda: pure_mcts_search_each(r, a.playouts, 1, 1.0, np.arange(G), seed=a.seed)}
        ms, moves = {k: [] for k in ways}, {}
        for rep in range(reps + 1):  # the first pass warms up
            for k in (list(ways) if rep % 2 == 0 else list(ways)[::-1]):
                t0 = time.perf_counter()
                moves[k] = ways[k]().moves.tobytes()
                if rep:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        row = {"G": G, "same_moves": moves["search"] == moves["search_each"]}
        for k in ways:
            row[k + "_ms_median"], row[k + "_ms_range"] = statistics.median(ms[k]), [min(ms[k]), max(ms[k])]
        print("per-root cost:", json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ways", default="lockstep,sequential,fights")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slow-rounds", type=int, default=0, help="rounds of sequential and fights (0: --rounds)")
    ap.add_argument("--game-amnt", type=int, default=100)
    ap.add_argument("--playouts", type=int, default=1600)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--no-per-root-cost", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    date = datetime.date.today().isoformat()
    out = Path(a.out) if a.out else ROOT / "profiles" / f"parameter_check_{date}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    ways = a.ways.split(",")
    doc = {"date": date, "host": socket.gethostname(), "argv": sys.argv[1:],
           "workload": f"n sweep: {len(pairings(N_VALUES))} pairings x {a.game_amnt} games, {a.playouts} playouts, "
                       "c 1.0, clock off", "legs": [], "ways": {}}
    results = {}
    for rnd in range(a.rounds):
        for way in (ways if rnd % 2 == 0 else ways[::-1]):
            if way != "lockstep" and rnd >= (a.slow_rounds or a.rounds):
                continue
            dt, plies, launches, res = run_way(way, a)
            leg = {"way": way, "round": rnd, "seconds": dt, "plies": plies, "launches": launches}
            print("leg:", json.dumps(leg), flush=True)
            doc["legs"].append(leg)
            if res is not None:
                if results and res != next(iter(results.values())):
                    raise SystemExit(f"{way} round {rnd}: results differ from {next(iter(results))}'s")
                results.setdefault(way, res)
            doc["ways"] = {w: summary([x for x in doc["legs"] if x["way"] == w]) for w in ways
                           if any(x["way"] == w for x in doc["legs"])}
            doc["lockstep_equals_sequential"] = len(results) == 2 or None
            out.write_text(json.dumps(doc, indent=1) + "\n")
    if not a.no_per_root_cost:
        doc["per_root_cost"] = per_root_cost(a)
        out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"out": str(out), "ways": doc["ways"]}), flush=True)


if __name__ == "__main__":
    main()
