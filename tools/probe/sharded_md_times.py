"""Times of the multi-depth exchange record of the camera-sharded runner at the benchmark geometry (7 cameras, one per rank: per = 1,
92 proposals per camera, E = 256, multi_depth topk = 3), in one job.

  python tools/probe/sharded_md_times.py [--out profiles/sharded_md/times.txt] [--rounds 7]

Recorded, not asserted (hipGraph replays, alternating repetitions in the same process):
  pack    far3d_proposal_pack_block of one camera's block (and of a block with one camera in two slots, and the empty block)  against
          the single-depth path's record construction, torch.cat (+ _pad with a padding slot), and against
          far3d_proposal_merge_blocks on the seven direct blocks (the same class of flat copies)
  merge   far3d_proposal_merge_blocks reading the seven gathered records in place (ops.md_block_views)  against  the same merge on
          the direct blocks; the results are compared bit for bit first.

The driver starts one child process per step, each under its own time limit, and stops at the first step that does not end cleanly."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "probe"))
from vov_family_times import graph_us  # noqa: E402

N, E, K_PROP, K_MD = 7, 256, 92, 3
STEP_LIMIT = 240
REPS = 5
DEV = "cuda:0"


def _block(seed, cams=1):
    """A camera block as camera_stage(block_rows=cams * 92) leaves it in the top-K mode (random rows: the kernels only move words)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    n = cams * K_PROP
    info = torch.randint(0, 50, (n, 2 * K_MD), generator=g, dtype=torch.int32)
    info[:, 0] = torch.arange(n, dtype=torch.int32) // K_PROP                       # the camera field, block-local
    return dict(ref2d=torch.rand(n, 3, generator=g).to(DEV), ctx=torch.randn(n, E + 1, generator=g).to(DEV),
                box2d=torch.rand(n, 4, generator=g).to(DEV), score2d=torch.rand(n, generator=g).to(DEV),
                sel_cnt=torch.full((cams,), K_PROP, dtype=torch.int32, device=DEV),
                md=dict(records=(torch.randint(0, 8, (n,), generator=g, dtype=torch.int32).to(DEV), info.to(DEV)),
                        img2lidar=torch.randn(cams, 4, 4, generator=g).to(DEV), sel_cap=0))


def _frame_out():
    import torch
    P = N * K_PROP
    out = (torch.empty((K_MD * P, 3), device=DEV), torch.empty((K_MD * P, E + 1), device=DEV), torch.empty((K_MD * P, 4), device=DEV),
           torch.empty((K_MD * P,), device=DEV))
    rec = (torch.empty((P,), dtype=torch.int32, device=DEV), torch.empty((P, 2 * K_MD), dtype=torch.int32, device=DEV))
    return out, rec, torch.empty((N,), dtype=torch.int32, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV), \
        torch.zeros((1,), dtype=torch.int32, device=DEV)


def _parts(blocks):
    return [dict(rows=(b["ref2d"], b["ctx"], b["box2d"], b["score2d"]), sel_cnt=b["sel_cnt"], first_cam=c, records=b["md"]["records"],
                 overflow=b.get("overflow"), count=K_PROP) for c, b in enumerate(blocks)]


def step_pack(rounds):
    import torch
    from far3d_amd import ops
    blocks = [_block(c) for c in range(N)]
    lay1, lay2 = ops.md_block_layout(1, K_PROP, E, K_MD), ops.md_block_layout(2, 2 * K_PROP, E, K_MD)
    rec1 = torch.empty((1, lay1["words"]), device=DEV)
    rec2 = torch.empty((1, lay2["words"]), device=DEV)
    out, rec, sel, m, ovf = _frame_out()
    parts = _parts(blocks)
    b0 = blocks[0]
    print(json.dumps(dict(kind="sizes", record_words_per1=lay1["words"], record_words_per2=lay2["words"],
                          single_depth_record_words=K_PROP * (E + 4))), flush=True)

    def cat1():                                                                   # ShardedFrame._camera_part, top-K, no padding slot
        return torch.cat([b0["ctx"], b0["ref2d"]], dim=1).view(1, K_PROP, E + 4)

    def cat2():                                                                   # the same with one camera in two slots: + _pad
        t = cat1()
        return torch.cat([t, torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)])

    fns = [("far3d_proposal_pack_block, per = 1, one camera", lambda: ops.proposal_pack_block(b0, rec1, lay1, count=K_PROP)),
           ("far3d_proposal_pack_block, per = 2, one camera", lambda: ops.proposal_pack_block(b0, rec2, lay2, count=K_PROP)),
           ("far3d_proposal_pack_block, per = 1, empty block", lambda: ops.proposal_pack_block(None, rec1, lay1)),
           ("single depth: torch.cat, per = 1", cat1),
           ("single depth: torch.cat + _pad (zeros, cat), per = 2", cat2),
           ("far3d_proposal_merge_blocks, 7 direct blocks", lambda: ops.proposal_merge_blocks(parts, out, sel, N * K_PROP, records_out=rec,
                                                                                               m_out=m, overflow_out=ovf))]
    for rep in range(REPS):
        row = dict(kind="pack", rep=rep)
        for name, fn in fns:
            row[name] = graph_us(fn, 10, rounds)[0]
        print(json.dumps(row), flush=True)


def step_merge(rounds):
    import torch
    from far3d_amd import ops
    blocks = [_block(c) for c in range(N)]
    lay = ops.md_block_layout(1, K_PROP, E, K_MD)
    buf = torch.empty((N, lay["words"]), device=DEV)
    for c, b in enumerate(blocks):
        ops.proposal_pack_block(b, buf[c:c + 1], lay, count=K_PROP)
    views = [ops.md_block_views(buf[c], lay, 1, c, 0) for c in range(N)]
    oa, ra, sa, ma, fa = _frame_out()
    ob, rb, sb, mb, fb = _frame_out()
    pa, pb = _parts(blocks), _parts(views)
    direct = lambda: ops.proposal_merge_blocks(pa, oa, sa, N * K_PROP, records_out=ra, m_out=ma, overflow_out=fa)
    records = lambda: ops.proposal_merge_blocks(pb, ob, sb, N * K_PROP, records_out=rb, m_out=mb, overflow_out=fb)
    direct(); records()
    torch.cuda.synchronize()
    P = N * K_PROP
    same = all(bool(torch.equal(x[:P], y[:P])) for x, y in zip(oa + ra, ob + rb)) and bool(torch.equal(sa, sb)) and bool(torch.equal(ma, mb))
    print(json.dumps(dict(kind="check", merge_from_records_equals_direct=same, rows=int(ma.item()))), flush=True)
    for rep in range(REPS):
        a, _ = graph_us(direct, 10, rounds)
        b, _ = graph_us(records, 10, rounds)
        print(json.dumps(dict(kind="merge", rep=rep, direct_us=a, records_us=b)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_md", "times.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        return step_pack(a.rounds) if a.step == "pack" else step_merge(a.rounds)
    rows = []
    for step in ("pack", "merge"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(a.rounds)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit("step %s did not finish within %d s; stopping" % (step, STEP_LIMIT))
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("step %s ended with status %d; stopping" % (step, r.returncode))
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        print("step %s done" % step, flush=True)
    write(rows, a.out)


def write(rows, path):
    L = ["Multi-depth exchange record of the camera-sharded runner: %d cameras, one per rank, %d proposals per camera, E = %d, topk = %d" %
         (N, K_PROP, E, K_MD), "hipGraph replays, median of the rounds, us per call", ""]
    for r in rows:
        if r["kind"] == "sizes":
            L.append("record: %d words (per = 1), %d words (per = 2); the single-depth record of a camera: %d words" %
                     (r["record_words_per1"], r["record_words_per2"], r["single_depth_record_words"]))
    mine = [r for r in rows if r["kind"] == "pack"]
    if mine:
        names = [k for k in mine[0] if k not in ("kind", "rep")]
        L += ["", "%d alternating repetitions" % len(mine)]
        for n in names:
            v = [r[n] for r in mine]
            L.append("  %-56s %s   mean %6.1f, spread %4.1f" % (n, " ".join("%6.1f" % x for x in v), sum(v) / len(v), max(v) - min(v)))
    for r in rows:
        if r["kind"] == "check":
            L += ["", "merge from the gathered records bit-equal to the merge from the blocks: %s (%d primary rows)" %
                  (r["merge_from_records_equals_direct"], r["rows"])]
    mine = [r for r in rows if r["kind"] == "merge"]
    if mine:
        L += ["far3d_proposal_merge_blocks, %d alternating repetitions" % len(mine), "  %3s %10s %10s" % ("rep", "direct", "records")]
        L += ["  %3d %10.1f %10.1f" % (r["rep"], r["direct_us"], r["records_us"]) for r in mine]
        a, b = [r["direct_us"] for r in mine], [r["records_us"] for r in mine]
        L.append("  mean direct %.1f, mean records %.1f; run-to-run spread %.1f" % (sum(a) / len(a), sum(b) / len(b), max(max(a) - min(a), max(b) - min(b))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
