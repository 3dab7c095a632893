"""Choose the LATTICE cases of tests/test_gpu_stage_spec.py by greedy set cover over the coverage ledger (tests/stage_lattice.py): small shapes that
between them launch every kernel instantiation the plan reaches in the ledger's envelope and that the older cases and the ladders leave out.
CPU only.  Prints the table as Python source; the committed table is this output (every data seed passed the CPU oracle test as printed) and one case added by hand,
t16_K232_d64_v: the statistics kernel without LDS shadows launched as two halves.

Candidates: N = 4000 (6000 where only that reaches the wave-pair chain); per NCT the cluster counts 16 NCT (a full last tile), 16 (NCT - 1) + 1 (one valid
lane in the last tile, K % 4 != 0: first-generation ridge kernels), 16 NCT - 8 and 16 NCT - 4 (inside a quad, K % 4 == 0) and the lowest K of an NCT that
has no kernel of its own size (129: nine tiles on the ten-tile kernel); d rotated over the list below; both sigma forms; one and two covariates."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stage_lattice as L  # noqa: E402

NCTS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 16)
D_BF = (50, 64, 32, 17, 48, 63, 16, 60, 24, 8, 3, 1, 28, 80, 100, 128, 96, 116)
D_F32 = (68, 76, 72, 65)
ENVS = ({}, {"HMX_CHAIN": "0"}, {"HMX_DOT": "f32"}, {"HMX_DOT": "f32", "HMX_CHAIN": "0"})


def k_choices(nct):
    prev = max([n for n in NCTS if n < nct], default=0)
    ks = {16 * nct: "full", 16 * (nct - 1) + 1: "lane", 16 * nct - 8: "quad", 16 * nct - 4: "quad"}
    if prev < nct - 1:
        ks[16 * prev + 1] = "low"
    return {k: v for k, v in ks.items() if k >= 2}          # (K = 1: a single cluster has no assignment to test)


def main():
    need, _ = L.envelope()
    need = set(need)
    have = set()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_stage_ref_cpu as T
    have |= T.ledger_of_existing_cases()
    print("# reachable %d, held by the older cases and the ladders %d" % (len(need), len(need & have)), file=sys.stderr)
    todo = need - have
    want_bounds = L.admitted_loop_bounds() - T.bounds_of_existing_cases()
    cands = []
    for env in ENVS:
        for nct in NCTS:
            for K, kind in k_choices(nct).items():
                for d in (D_F32 if "HMX_DOT" not in env else ()) + D_BF:
                    for C_ in (1, 2):
                        for usig in (1, 0):
                            for N in (4000, 6000):
                                shape, items = L.even_shape(N, d, C_, usig)
                                got, p = L.launches(N, K, shape, items, env, "stages")
                                if got:
                                    cands.append(dict(N=N, d=d, C=C_, usig=usig, K=K, kind=kind, nct=nct, env=env, got=set(got), credit=got, p=p,
                                                      bounds=L.loop_bounds(got, p)))
    chosen, used_kind, used_d = [], {}, {}
    while todo or want_bounds:
        def score(c):
            return (len(c["got"] & todo), len(c["bounds"] & want_bounds), -used_kind.get((c["nct"], c["kind"]), 0), -len(c["env"]), -used_d.get(c["d"], 0), -c["N"], c["C"] == 1 + len(chosen) % 2)
        best = max(cands, key=score)
        if not (best["got"] & todo or best["bounds"] & want_bounds):
            break
        chosen.append(best)
        todo -= best["got"]
        want_bounds -= best["bounds"]
        used_kind[(best["nct"], best["kind"])] = used_kind.get((best["nct"], best["kind"]), 0) + 1
        used_d[best["d"]] = used_d.get(best["d"], 0) + 1
    # every NCT at a full tile, at one valid lane, inside a quad and -- where the next smaller kernel is more than a tile away -- at its lowest K
    for nct in NCTS:
        for kind in ("full", "lane", "quad", "low"):
            if not used_kind.get((nct, kind)) and any(k >= 2 for k, v in k_choices(nct).items() if v == kind):
                best = max((c for c in cands if c["nct"] == nct and c["kind"] == kind and not c["env"] and c["N"] == 4000), key=lambda c: (-used_d.get(c["d"], 0), c["usig"]))
                chosen.append(best)
                used_kind[(nct, kind)] = 1
                used_d[best["d"]] = used_d.get(best["d"], 0) + 1
    print("# not reached by any candidate:", sorted(todo), sorted(want_bounds), file=sys.stderr)
    chosen.sort(key=lambda c: (c["nct"], c["K"], c["d"], c["usig"], sorted(c["env"].items())))
    print("LATTICE = {")
    for i, c in enumerate(chosen):
        p, tiles = c["p"], {kind: v[1:] for v, kind in c["credit"].items() if v[0] == "k_tile" and kind in ("head", "update", "chain")}
        ridge = {kind: v[1:] for v, kind in c["credit"].items() if v[0] in ("stats", "apply")}
        on_chain = int(p["chain_ok"] or p["chain_pair"])
        name = "t%02d_K%d_d%d_%s%s%s" % (c["nct"], c["K"], c["d"], "u" if c["usig"] else "v", "_c2" if c["C"] == 2 else "",
                                         "".join("_" + k[4:].lower() + v for k, v in sorted(c["env"].items())))
        path = dict(chain=on_chain, chain_pair=p["chain_pair"], usig=p["usig"], upd_wps=p["upd_wps"], dot_bf=p["dot_bf"], moe_mfma=p["moe_mfma"], host=0)
        print("    %r: (%d, %d, %r, %d, %r, %r, %d,\n        %r,\n        %r)," % (
            name, c["N"], c["d"], L.ENVELOPE_LEVELS[c["C"]], c["K"], "u" if c["usig"] else "v", c["env"], 200 + i, path, dict(tiles, **ridge)))
    print("}")
    print("# %d cases" % len(chosen), file=sys.stderr)


if __name__ == "__main__":
    main()
