#!/usr/bin/env python3
"""Randomised file-boundary sweep (build container: needs oracle/_ref): random hierarchies written in the reference's
formats, read back by (a) the REFERENCE's read_grid through oracle/ref_harness.cpp, (b) the oracle's reader, (c) the
library's reader (mgcfd_mesh_load) — sizes, edge arrays (class order, signs), volumes and coordinates must be identical.
--record FILE keeps what (a) read for every seed and level (sizes, SHA-256 of each array's bits) in FILE; --golden FILE checks
(b) and (c) against such a record instead, so no oracle/_ref is needed (tests/golden/fuzz_reader_reference.json).
    python tools/fuzz_reader.py [--seeds 60] [--first 0] [--record FILE | --golden FILE]"""
import argparse, hashlib, json, os, shutil, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd")); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=60)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--record", metavar="FILE", help="also write what the reference read for every seed into FILE (merged with what it holds)")
    ap.add_argument("--golden", metavar="FILE", help="compare against what the reference read, recorded in FILE, instead of calling it")
    args = ap.parse_args()
    import numpy as np
    import mgcfd
    from mgcfd import meshgen
    import oracle_py as O
    import fuzz_parity
    if not args.golden and not O.have_reference():
        raise SystemExit("oracle/_ref is missing: run oracle/build_ref.sh first")
    ref = None if args.golden else O.load_reference()
    golden = json.load(open(args.golden))["seeds"] if args.golden else None
    record = json.load(open(args.record))["seeds"] if args.record and os.path.exists(args.record) else {}

    def digest(a, dtype):
        return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()
    bad = 0
    for seed in range(args.first, args.first + args.seeds):
        rng = np.random.default_rng(7000 + seed)
        while True:
            kind, name, mg, _ = fuzz_parity.make_case(rng)
            if max(l.nel for l in mg.levels) <= 3000 and all(mg.levels[k + 1].nel <= mg.levels[k].nel for k in range(len(mg.levels) - 1)):
                break
        d = tempfile.mkdtemp(prefix="mgcfd_rd_")
        try:
            meshgen.write_input(mg, d)
            info = O.parse_input_dat(os.path.join(d, "input.dat"))
            n_levels = len(info["levels"])
            tag = f"seed {seed}: {kind} {name} {[l.nel for l in mg.levels]}"
            if golden is not None:
                if golden.get(str(seed), {}).get("tag") != tag:
                    raise SystemExit(f"{args.golden} holds no record of {tag!r}")
            else:
                ref.ref_init(n_levels, info["mesh_variant"])
            ours = mgcfd.Mesh("input.dat", d)
            oc = O.OracleCase.from_input_dat(os.path.join(d, "input.dat"))
            problems = []
            read = []
            for l in range(n_levels):
                if golden is not None:
                    want = golden[str(seed)]["levels"][l]
                else:
                    sizes = np.zeros(8, dtype=np.int64)
                    ref.ref_set_level(l)
                    ref.ref_read_grid(os.path.join(d, info["levels"][l]).encode(), O.ptr(sizes))
                    nel, n_edges = int(sizes[0]), int(sizes[1])
                    vol, edges, coords = np.zeros(nel), np.zeros(n_edges, dtype=O.EDGE_DTYPE), np.zeros((nel, 3))
                    ref.ref_grid_copy(O.ptr(vol), O.ptr(edges), O.ptr(coords))
                    want = {"sizes": [int(v) for v in sizes[:5]], "edges_sha256": digest(edges, O.EDGE_DTYPE),
                            "volumes_sha256": digest(vol, "<f8"), "coords_sha256": digest(coords, "<f8")}
                    read.append(want)
                L = ours.level(l)
                sizes = want["sizes"]
                if (L["nel"], L["n_internal"], L["n_boundary"], L["n_wall"]) != tuple(sizes[i] for i in (0, 2, 3, 4)):
                    problems.append(f"level {l} sizes {(L['nel'], L['n_internal'], L['n_boundary'], L['n_wall'])} vs {sizes}")
                    continue
                if digest(L["edges"], O.EDGE_DTYPE) != want["edges_sha256"]: problems.append(f"level {l} edges (library)")
                if digest(oc.edges(l), O.EDGE_DTYPE) != want["edges_sha256"]: problems.append(f"level {l} edges (oracle)")
                if digest(L["volumes"], "<f8") != want["volumes_sha256"]: problems.append(f"level {l} volumes")
                if n_levels > 1 and digest(L["coords"], "<f8") != want["coords_sha256"]: problems.append(f"level {l} coords")
            if golden is None:
                record[str(seed)] = {"tag": tag, "levels": read}
            ours.close(); oc.close()
            print(f"{tag}: " + ("ok" if not problems else "MISMATCH " + "; ".join(problems)), flush=True)
            bad += 1 if problems else 0
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if args.record:
        with open(args.record, "w") as f:
            json.dump({"what": "what the reference's read_grid read in tools/fuzz_reader.py, per seed and level (python tools/fuzz_reader.py --record)",
                       "seeds": dict(sorted(record.items(), key=lambda kv: int(kv[0])))}, f, indent=1)
    print("mismatches:", bad)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
