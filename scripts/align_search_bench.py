"""Times the score of a pose search (csrc/align_score.hip, ops.align_score) and the whole search (point_sam_amd/align.py: search) next to the only way the
same counts could be had before: one ops.align_step per pose, each followed by a read of sums[0].

    python scripts/align_search_bench.py [--repeats 20] [--loop-repeats 3] [--limit 300] [--out FILE.json]

The fixture is tests/align_search_reference.py's: 6000 sources on three plane patches and a sphere, the queries a second sample cut to x < 0.1 and given
in a frame 132 degrees (yaw) or 130 degrees (skew axis) away.  Two sizes:
    small   P = 1 944  (72 yaw steps x 27 offsets), 512 queries scored
    large   P = 62 208 (96 x 24 rotations x 27 offsets), 1 024 queries scored
Each size runs in a child process of its own under a time limit of `--limit` seconds; the first one that fails or runs out of time ends the run.

  score       ops.align_score with the poses already on the device: device-event time, median of `--repeats` after two warm-up calls, with min and max
  score_host  the same from host poses (validation, upload) to the counts on the host: wall time
  loop        P x (ops.align_step, int(sums[0])): wall time, median of `--loop-repeats` after one warm-up pass.  The counts must be equal, all P
  search      align.search end to end (scoring, one host read, `keep` refinements): wall time
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"small": dict(kind="yaw", sample=512), "large": dict(kind="so3", sample=1024)}


def run_case(name, repeats, loop_repeats):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import align_search_reference as S
    from scene_bench import event, stat, wall
    from point_sam_amd import align, ops

    case = CASES[name]
    truth = S.YAW_TRUTH if case["kind"] == "yaw" else S.SO3_TRUTH
    a, b = S._case(truth, True)
    icp = align.AlignConfig(**S.ICP)
    grid = dict(rotations="yaw", yaw_steps=S.YAW_STEPS) if case["kind"] == "yaw" else dict(rotations="so3", axes=S.SO3_AXES, rolls=S.SO3_ROLLS)
    cfg = align.SearchConfig(offsets=1, offset_step=0.1, sample=case["sample"], radius=S.SCORE_RADIUS, keep=S.KEEP, **grid)
    src, qry = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    index = ops.transfer_index(src, icp.radius)
    pick = torch.from_numpy(align.sample_positions(len(b), cfg.sample)).cuda()
    sample = qry.index_select(0, pick).contiguous()
    poses = align.candidate_poses(cfg, a.astype(np.float64).mean(0), sample.double().mean(0).cpu().numpy())
    words = torch.from_numpy(ops.transfer_poses(poses)).cuda()
    res = dict(case=name, poses=len(poses), sample=sample.shape[0], sources=len(a), queries=len(b), radius=S.SCORE_RADIUS, index_radius=icp.radius,
               chunk=ops.ALIGN_SCORE_POSES, repeats=repeats, loop_repeats=loop_repeats)

    counts = ops.align_score(index, sample, words, cfg.radius).cpu().numpy()
    score = [event(lambda: ops.align_score(index, sample, words, cfg.radius))[1] for _ in range(repeats + 2)][2:]
    host = [wall(lambda: ops.align_score(index, sample, poses, cfg.radius).cpu())[1] for _ in range(min(repeats, 5) + 1)][1:]

    def loop():
        return [int(ops.align_step(index, sample, p, cfg.radius)[0]) for p in poses]
    looped = loop()                                                    # the warm-up pass, and the check
    assert counts.tolist() == looped, "ops.align_score and the loop over ops.align_step disagree"
    loop_ms = [wall(loop)[1] for _ in range(loop_repeats)]
    out = align.search(index, qry, cfg, icp)
    search = [wall(lambda: align.search(index, qry, cfg, icp))[1] for _ in range(min(repeats, 3))]
    rot, tr = S.A.pose_error(out.pose, truth)
    res.update(best_count=int(counts.max()), median_count=float(np.median(counts)), score_ms=stat(score), score_host_ms=stat(host), loop_ms=stat(loop_ms),
               loop_over_score=round(stat(loop_ms)["median"] / stat(score)["median"], 1),
               loop_over_score_host=round(stat(loop_ms)["median"] / stat(host)["median"], 1),
               poses_per_ms=round(len(poses) / stat(score)["median"], 1), search_ms=stat(search),
               search=dict(pairs=out.pairs, rms=round(out.rms, 6), converged=out.converged, chosen=out.search.chosen, rotation_error=rot, translation_error=tr,
                           refined=[(c["pose_index"], c["count"], c["pairs"]) for c in out.search.candidates]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:                                              # the child: one size, one JSON line
        print(json.dumps(run_case(args.case, args.repeats, args.loop_repeats)), flush=True)
        return 0
    out = []
    for name in ("small", "large"):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--repeats", str(args.repeats), "--loop-repeats", str(args.loop_repeats)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.limit} s; nothing more is started", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; nothing more is started\n{r.stderr[-4000:]}", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)
        out.append(res)
        if args.out:                                           # after every size: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
