#!/usr/bin/env python3
"""The rearrangement learning run (tools/nav2d_rearr_learning.py: PPOTrainer, PointNavResNetPolicy with ResNet18 on head_depth and
the three fused sensors, start_holding, turn_angle 30, 32 envs x 32 steps at 64 x 64) in both distance modes at K = 3 obstacles, the
same seeds and the same budget for both.  Reports, per mode and seed, the return, the success and the final object_to_goal_distance
of the first and of the last five updates, and the means over the seeds.  The return and object_to_goal_distance of the geodesic mode
are measured along the shortest path, those of the Euclidean mode along the straight line: in a world with detours the same behaviour
gives the geodesic mode the larger distance.  No threshold is held here; the numbers are reported as measured.
usage: python tools/nav2d_rearr_geo_learning.py [--updates U] [--seeds S [S ...]] [--obstacles K] [--max-steps E]"""
import argparse
import importlib.util
import os
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("nav2d_rearr_learning", os.path.join(HERE, "nav2d_rearr_learning.py"))
base = importlib.util.module_from_spec(spec)
spec.loader.exec_module(base)

KEYS = ("return_first", "return_last", "success_first", "success_last", "distance_first", "distance_last", "z", "seconds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--seeds", type=int, nargs="+", default=[100, 101])
    ap.add_argument("--obstacles", type=int, default=3)
    ap.add_argument("--max-steps", type=int, default=48)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_rearr_geo_learning needs a GPU"
    runs = {}
    for distance in ("euclidean", "geodesic"):
        for seed in a.seeds:
            with tempfile.TemporaryDirectory() as folder:
                r = base.learning_run(folder, seed=seed, updates=a.updates, max_steps=a.max_steps, obstacles=a.obstacles,
                                      distance=distance)
            runs[(distance, seed)] = r
            print(f"{distance:9s} seed {seed}:", {k: round(float(r[k]), 4) for k in KEYS}, flush=True)
    for distance in ("euclidean", "geodesic"):
        mean = {k: sum(float(runs[(distance, s)][k]) for s in a.seeds) / len(a.seeds) for k in KEYS}
        print(f"{distance:9s} mean of {len(a.seeds)} seeds, K = {a.obstacles}, {a.updates} updates: final success {mean['success_last']:.3f}, "
              f"final object_to_goal_distance {mean['distance_last']:.3f} m (first five updates {mean['distance_first']:.3f} m), "
              f"return {mean['return_first']:.3f} -> {mean['return_last']:.3f}, z {mean['z']:.1f}, {mean['seconds']:.1f} s")


if __name__ == "__main__":
    main()
