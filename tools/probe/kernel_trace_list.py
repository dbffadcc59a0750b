"""The ordered launch list of a rocprofv3 kernel trace (csv): one line `kernel name | grid | workgroup size` per dispatch, in dispatch
order, and its sha256 and length -- what two checkouts that must issue the same launches are compared on.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/probe/decoder_body_digest.py --trace [--root CHECKOUT]
  python tools/probe/kernel_trace_list.py DIR/run_kernel_trace.csv [--out launches.txt]"""
import argparse
import csv
import hashlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with open(args.csv, newline="") as f:
        rows = list(csv.DictReader(f))
    order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))
    dims = lambda r, what: "x".join(r[k] for k in sorted(r) if k.startswith(what))
    text = "".join("%s | %s | %s\n" % (r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size")) for r in rows)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print("%s  %d launches  %s" % (hashlib.sha256(text.encode()).hexdigest(), len(rows), args.csv))


if __name__ == "__main__":
    main()
