"""Same-box A/B of whole trees: runs `bench.py` of every tree alternately (rounds x trees) and prints tiles/s and the per-class GPU times.
    python tools/ab_bench.py --rounds 2 --workload encdec .ab/r05 .
    python tools/ab_bench.py --rounds 3 --scene .ab/parent .ab/parent .     # bench.py's scene leg (ms per 2048-px scene) instead; naming a
                                                                             # tree twice gives the same-tree spread to judge a difference by
Trees are checkouts / exports of this repository with their library built in place (git archive <commit> | tar -x -C .ab/<name>;
python -m sam_road_amd.build inside).  .ab/ is git-ignored but travels to the GPU box with gpurun."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("trees", nargs="+")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--workload", default="encdec")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--scene", action="store_true", help="compare the scene block (ms_per_scene, lower is better) instead of tiles/s")
ap.add_argument("--scenes", type=int, default=16)
args = ap.parse_args()
slots = [(i, t) for i, t in enumerate(args.trees)]          # a tree named twice is two slots
res = {s: [] for s in slots}
for r in range(args.rounds):
    for slot in slots:
        t = slot[1]
        env = {k: v for k, v in os.environ.items() if k != "SRH_LIB_PATH"}
        # the per-class times come from the roofline leg, which only a --full run has (trees from before --full run it by default)
        full = ["--full"] if "--full" in open(os.path.join(t, "bench.py")).read() else []
        if args.scene:
            out = subprocess.run([sys.executable, "bench.py", "--steps", "5", "--warmup", "2"] + full + ["--scenes", str(args.scenes),
                                  "--no-cpu-baseline", "--no-reference-gpu", "--no-sustained", "--no-roofline", "--no-workloads"],
                                 capture_output=True, text=True, env=env, cwd=t)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            sc = json.loads(line[-1]).get("scene", {}) if line else {}
            if "ms_per_scene" not in sc:
                print(f"{t} round {r}: FAILED\n{out.stderr[-2000:]}\n{sc}", flush=True)
                continue
            res[slot].append(sc["ms_per_scene"])
            print(f"{t} (slot {slot[0]}) round {r}: {sc['ms_per_scene']:.2f} ms per scene over {sc.get('scenes')} scenes", flush=True)
            continue
        out = subprocess.run([sys.executable, "bench.py", "--workload", args.workload, "--steps", str(args.steps), "--warmup", "5"] + full +
                             ["--no-cpu-baseline", "--no-reference-gpu", "--no-sustained", "--no-scene", "--no-workloads"],
                             capture_output=True, text=True, env=env, cwd=t)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if not line:
            print(f"{t} round {r}: FAILED\n{out.stderr[-2000:]}", flush=True)
            continue
        js = json.loads(line[-1])
        cls = js.get("roofline", {}).get("by_class_ms_per_step", {})
        res[slot].append(js["value"])
        print(f"{t} round {r}: {js['value']:.1f} tiles/s  dominant {js.get('roofline', {}).get('dominant_kernel', {}).get('frac')}  {cls}", flush=True)
unit = "ms per scene" if args.scene else "tiles/s"
for (i, t), v in res.items():
    if v:
        print(f"{t} (slot {i}): mean {sum(v) / len(v):.2f} {unit} over {len(v)} runs ({', '.join('%.2f' % x for x in v)}), spread {max(v) - min(v):.2f}")
