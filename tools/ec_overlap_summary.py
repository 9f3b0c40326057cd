"""How far the front kernels of one ES256 batch (k_prep, k_ec_scalar_batch) run
under the other lane's k_ec_point in a rocprofv3 --kernel-trace CSV of the
plain streamed headline (python bench.py), and how long each kernel takes when
it overlaps against when it runs alone (bench.py's synchronous warm-up runs).
usage: python tools/ec_overlap_summary.py kt_kernel_trace.csv [out.json]"""
import csv
import json
import statistics
import sys

MIN_NS = 50_000          # the headline's launches; key staging and table kernels are other names or far shorter
NAMES = {"k_prep<": "prep", "k_ec_scalar_batch": "scalar", "k_ec_point<": "point"}


def kind(name):
    for k, v in NAMES.items():
        if k in name:
            return v
    return None


def main(path, out=None):
    ev = []
    for r in csv.DictReader(open(path)):
        k = kind(r["Kernel_Name"])
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if k and e - s >= MIN_NS:
            ev.append((s, e, k, r["Queue_Id"]))
    ev.sort()
    points = [(s, e, q) for s, e, k, q in ev if k == "point"]
    fronts = [(s, e, q) for s, e, k, q in ev if k != "point"]

    def under(s, e, q, others):
        # part of [s, e) covered by an interval of `others` on another queue
        return sum(max(0, min(e, pe) - max(s, ps)) for ps, pe, pq in others if pq != q and pe > s and ps < e)

    res = {"source": "rocprofv3 --kernel-trace, python bench.py (no counters in the run)", "kernels": {}}
    for k in ("prep", "scalar", "point"):
        alone, over, frac = [], [], []
        for s, e, kk, q in ev:
            if kk != k:
                continue
            f = under(s, e, q, points if k != "point" else fronts) / (e - s)
            if f < 0.02:
                alone.append((e - s) / 1e6)
            else:
                over.append((e - s) / 1e6)
                frac.append(f)
        med = lambda v: round(statistics.median(v), 4) if v else None
        res["kernels"][k] = {
            "alone_n": len(alone), "alone_ms_median": med(alone),
            "overlapped_n": len(over), "overlapped_ms_median": med(over),
            ("frac_under_other_lane_point" if k != "point" else "frac_with_other_lane_front_median"): med(frac),
        }
    # steady state: per step, the wall time from one point kernel's end to the next one's end
    ends = sorted(e for _, e, _ in points)
    gaps = [(b - a) / 1e6 for a, b in zip(ends, ends[1:])]
    if gaps:
        res["point_end_to_end_ms_median"] = round(statistics.median(gaps), 4)
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        open(out, "w").write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None)
