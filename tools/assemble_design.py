#!/usr/bin/env python
"""DESIGN.md = docs/design_parts/*.md in file order (and README.md = docs/readme_template.md), with the @@KEY@@ placeholders filled from the committed evidence under profiles/<tag>_*
(python tools/assemble_design.py [tag], default r6; no GPU needed).  A key whose source file is missing is left as `n/a (file)` and reported."""
import io
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")
TAG = sys.argv[1] if len(sys.argv) > 1 else "r6"
missing = []


def line(fn):
    try:
        return json.loads(open(os.path.join(P, fn)).read().strip().splitlines()[-1])
    except Exception:
        missing.append(fn)
        return None


def js(fn):
    try:
        return json.load(open(os.path.join(P, fn)))
    except Exception:
        missing.append(fn)
        return None


def fmt(x, nd=1):
    return ("%." + str(nd) + "f") % x


vals = {}
d = line(TAG + "_bench_default.json")
if d:
    also = d.get("also") or {}
    vals["DEF_MS"] = fmt(d["ms_per_step"], 2)
    vals["DEF_CPS"] = fmt(d["value"] / 1e6, 1)
    vals["STEP_US"] = fmt(d["roofline"]["avg_block_step_us"], 1)
    vals["FRAC"] = fmt(d["roofline"]["frac"], 3)
    vals["FRAC_NOM"] = fmt(d["roofline"]["nominal"]["frac"], 3)
    ph = d["config"]["gpu_phase_ms_per_step"]
    vals["PHASES_DEF"] = ", ".join("%s %s" % (k, fmt(v, 2)) for k, v in ph.items() if isinstance(v, (int, float)))
    ra = also.get("reference_arith")
    if ra:
        vals["REF_MS"] = fmt(ra["ms_per_step"], 1)
        vals["REF_CPS"] = fmt(ra["cells_per_s"] / 1e6, 1)
        vals["PHASES_REF"] = ", ".join("%s %s" % (k, fmt(v, 1)) for k, v in ra["gpu_phase_ms_per_step"].items())
    r2 = also.get("reference_arith_2")
    if r2 and "ms_per_step" in r2:
        vals["REF2_MS"] = fmt(r2["ms_per_step"], 1)
        vals["REF2_CPS"] = fmt(r2["cells_per_s"] / 1e6, 1)
    for key, leg in (("10M", "10M_one_gpu"), ("SHARE", "configs3_share_1p25M"), ("C5_1M", "c5_shape_1M"), ("PBMC", "pbmc30k")):
        if leg in also and "ms_per_step" in also[leg]:
            vals[key + "_MS"] = fmt(also[leg]["ms_per_step"], 1)
            if key == "10M":
                vals["10M_CPS"] = fmt(also[leg]["cells_per_s"] / 1e6, 0)
c5 = line(TAG + "_bench_c5_5M.json")
if c5:
    vals["C5_5M_MS"] = fmt(c5["ms_per_step"], 1)
for key, fn in (("C5_5M", TAG + "_parity_c5_5M.json"), ("C4_10M", TAG + "_parity_c4_10M.json")):
    t = js(fn)
    if t:
        pr = t["pairs"]
        ga, rf = pr["gpu_vs_oracle_accurate"], pr["gpu_ref_arith_vs_oracle_faithful"]
        row = "%.1e / %d clear flips · %.1e / %d" % (ga["Z_rel"], ga["argmax_diff_margin_ge_1e-5"], rf["Z_rel"], rf["argmax_diff_margin_ge_1e-5"])
        if "oracle_faithful_liberty1_vs_oracle_faithful" in pr:
            lb = pr["oracle_faithful_liberty1_vs_oracle_faithful"]
            row += " · %.1e / %d" % (lb["Z_rel"], lb["argmax_diff_margin_ge_1e-5"])
        row += " (GPU %.2f s / %.2f s, oracle %.0f s)" % (t["seconds"]["gpu"], t["seconds"]["gpu_ref_arith"], t["seconds"]["oracle_faithful"])
        vals[key + "_ROWS"] = row
        if key == "C5_5M":
            vals["C5_5M_REF"] = fmt(t["seconds"]["gpu_ref_arith"], 2)
        else:
            vals["10M_REF_S"] = fmt(t["seconds"]["gpu_ref_arith"], 2)
            vals["10M_Z"] = "%.1e" % ga["Z_rel"]
            vals["10M_REF_Z"] = "%.1e" % rf["Z_rel"]
try:
    tab = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "roofline_all_kernels.py"), TAG], capture_output=True, text=True, timeout=120)
    if tab.returncode == 0:
        vals["ROOFLINE_TABLE"] = tab.stdout.strip()
    else:
        missing.append("roofline_all_kernels.py: " + tab.stderr.strip()[-200:])
except Exception as e:       # noqa: BLE001
    missing.append("roofline_all_kernels.py: %s" % e)

try:
    tab = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scaling_prediction.py"), TAG], capture_output=True, text=True, timeout=120)
    if tab.returncode == 0:
        vals["SCALING_TABLE"] = tab.stdout.strip()
    else:
        missing.append("scaling_prediction.py: " + (tab.stderr.strip() or tab.stdout.strip())[-200:])
except Exception as e:       # noqa: BLE001
    missing.append("scaling_prediction.py: %s" % e)

ab = js("launch_path_ab.json")      # parent and change alternating, five plain bench lines each
if ab:
    side = {k: [r["ms_per_step"] for r in ab["runs"] if r["side"] == k] for k in ("parent", "change")}
    mean = {k: sum(v) / len(v) for k, v in side.items()}
    sd = {k: (sum((x - mean[k]) ** 2 for x in v) / (len(v) - 1)) ** 0.5 for k, v in side.items()}
    diff, bar = mean["parent"] - mean["change"], 3 * max(sd.values())
    vals["LP_AB"] = ("parent %s ms per step (mean of %d, standard deviation %s), change %s (%s): %s ms or %s %% less; three times the larger standard deviation is %s ms -- %s."
                     % (fmt(mean["parent"], 3), len(side["parent"]), fmt(sd["parent"], 3), fmt(mean["change"], 3), fmt(sd["change"], 3), fmt(diff, 3), fmt(100 * diff / mean["parent"], 1),
                        fmt(bar, 3), "the gain counts" if diff > bar else "the difference does NOT clear that bar"))

lb = line("r7_lisi_bench.json")      # tools/lisi_bench.py
if lb:
    kt = "; ".join("%s %.1f ms" % (k["kernel"].split("(")[0].replace("void hmx::", ""), k["total_ms"]) for k in lb.get("kernel_trace", []))
    vals["LISI_MEASURED"] = ("**Measured** (`profiles/r7_lisi_bench.json`, median of %d): %.0f ms per call, of which the neighbour search %.0f ms and the LISI stage %.1f ms"
                             "; the GEMM bound is %.0f ms, so the search runs at %.2f of the fp32 matrix-core peak. Kernel trace (one run): %s."
                             % (lb["repeats"], lb["ms_median"], lb["median_ms_knn"], lb["median_ms_lisi"], lb["bound_ms_gemm_fp32_mfma"],
                                lb["bound_ms_gemm_fp32_mfma"] / lb["median_ms_knn"], kt or "not collected"))
else:
    vals["LISI_MEASURED"] = "**Not measured yet**: `profiles/r7_lisi_bench.json` (written by `tools/lisi_bench.py` on an MI355X) is not in the tree."
sb = line(TAG + "_silhouette_bench.json")      # tools/silhouette_bench.py
if sb:
    rows = []
    for r in sb["sizes"]:
        lab, bat, kn = r["label"], r["batch_within_label"], r["knn"]
        rows.append("N = %s: label silhouette %.0f ms (GEMM bound %.0f ms, %.2f of the fp32 matrix-core peak; square roots %.0f ms), batch silhouette within the "
                    "cell types %.0f ms (%.3f N² pairs, GEMM bound %.1f ms), `hmx_knn` with k = %d %.0f ms — the label silhouette takes %.2f of the kNN's time"
                    % ("{:,}".format(r["cells"]).replace(",", " "), lab["ms_median"], lab["bound_ms_gemm_fp32_mfma"], lab["bound_ms_gemm_fp32_mfma"] / lab["ms_median"],
                       lab["bound_ms_sqrt"], bat["ms_median"], bat["pairs"] / float(r["cells"]) ** 2, bat["bound_ms_gemm_fp32_mfma"], sb["knn_k"], kn["ms_median"],
                       r["label_over_knn"]))
    vals["SIL_MEASURED"] = ("**Measured** (`profiles/%s_silhouette_bench.json`, one MI355X, median of %d calls, host time around the call with the sort and the "
                            "copies in it): %s." % (TAG, sb["repeats"], "; ".join(rows)))
else:
    vals["SIL_MEASURED"] = ("**Not measured yet**: `profiles/%s_silhouette_bench.json` (written by `tools/silhouette_bench.py` on an MI355X) is not in the tree." % TAG)
cb = line(TAG + "_confidence_bench.json")      # tools/confidence_bench.py
if cb:
    rm, so, sd = cb["reference_moments"], cb["mapping_confidence_score_only"], cb["mapping_confidence_score_and_dist"]
    vals["CONF_MEASURED"] = ("**Measured** (`profiles/%s_confidence_bench.json`, one MI355X, %s cells x %d PCs, K = %d, median of %d calls, host time around the "
                             "call): `reference_summary(moments=\"orig\")` %.1f ms, of which `hmx_reference_moments` %.1f ms (pass B's MFMA bound %.1f ms; the rest is the plain summary), "
                             "the confidence of the mapped query %.1f ms for the score alone "
                             "(MFMA bound %.1f ms, the host's Cholesky factors and the copies in it) and %.1f ms with the distance matrix."
                             % (TAG, "{:,}".format(cb["cells"]).replace(",", " "), cb["d"], cb["K"], cb["repeats"], rm["ms_median"], rm["timer_ms_median"], rm["bound_ms_fp32_mfma"],
                                so["ms_median"], so["bound_ms_fp32_mfma"], sd["ms_median"]))
else:
    vals["CONF_MEASURED"] = ("**Not measured yet**: `profiles/%s_confidence_bench.json` (written by `tools/confidence_bench.py` on an MI355X) is not in the tree." % TAG)
pb = line(TAG + "_project_bench.json")      # tools/project_bench.py
if pb:
    dv, ho = pb["device_resident"], pb["host_resident"]
    vals["PROJECT_MEASURED"] = ("**Measured** (`profiles/%s_project_bench.json`, one MI355X, %s cells x %d genes, %.0f stored counts per cell, G = %d, d = %d, PCs left in "
                                "HBM, median of %d calls by the library's timer): device-resident %.1f ms (two sweeps from HBM would take %.1f ms, one %.1f ms: the call moves "
                                "%.2f TB/s counted as one sweep), host-resident %.0f ms in %d slabs, %.1f GB/s across PCIe with the host's validation pass in it; "
                                "the two give the same bits: %s."
                                % (TAG, "{:,}".format(pb["cells"]).replace(",", " "), pb["G_all"], pb["nnz_per_cell"], pb["G"], pb["d"], pb["repeats"], dv["timer_ms_median"],
                                   dv["bound_ms_two_sweeps_from_hbm"], dv["bound_ms_one_sweep_from_hbm"], dv["bytes_per_s_of_one_sweep"] / 1e12, ho["timer_ms_median"],
                                   ho["slabs"], ho["bytes_per_s"] / 1e9, "yes" if pb["host_equals_device_bits"] else "NO"))
else:
    vals["PROJECT_MEASURED"] = ("**Not measured yet**: `profiles/%s_project_bench.json` (written by `tools/project_bench.py` on an MI355X) is not in the tree." % TAG)
qb = line("pca_bench.json")      # tools/pca_bench.py
if qb:
    dv, ho, bd = qb["device_resident"], qb["host_resident"], qb["bound_ms"]
    vals["PCA_MEASURED"] = ("**Measured** (`profiles/pca_bench.json`, one MI355X, %s cells x %d genes, %.0f stored counts per cell, G = %d, k = %d, %s contributing entries, "
                            "median of %d calls by the library's timers): device-resident `gene_stats` %.1f ms (bound %.1f ms), `prepare` %.1f ms (bound %.1f ms), one `apply` %.1f ms "
                            "(lists %.1f ms + row gathers %.1f ms if they streamed from HBM); host-resident `gene_stats` %.0f ms, `prepare` %.0f ms in %d slabs per sweep, `apply` %.1f ms; "
                            "host- and device-resident input give the same bits: %s."
                            % ("{:,}".format(qb["cells"]).replace(",", " "), qb["G_all"], qb["nnz_per_cell"], qb["G"], qb["k"], "{:,}".format(qb["pca_entries"]).replace(",", " "),
                               qb["repeats"], dv["gene_stats_ms"], bd["gene_stats_device"], dv["prepare_ms"], bd["prepare_device"], dv["apply_ms"], bd["apply_lists"],
                               bd["apply_row_gathers_from_hbm"], ho["gene_stats_ms"], ho["prepare_ms"], ho["slabs"], ho["apply_ms"], "yes" if qb["host_equals_device_bits"] else "NO"))
else:
    vals["PCA_MEASURED"] = "**Not measured yet**: `profiles/pca_bench.json` (written by `tools/pca_bench.py` on an MI355X) is not in the tree."
gb = line("group_stats_bench.json")      # tools/group_stats_bench.py
if gb:
    rows = []
    for where in ("device_resident", "host_resident"):
        r = gb.get(where)
        if r:
            rows.append("%s `gene_stats` %.1f ms (run-to-run spread, (max - min) / median, %.1f %% over %d calls)%s; grouped: %s"
                        % (where.replace("_", "-"), r["gene_stats_ms"], 100.0 * r["gene_stats_spread"], len(r["gene_stats_ms_all"]),
                           " in %d slabs" % r["slabs"] if r["slabs"] > 1 else "",
                           ", ".join("B = %s %.1f ms (ratio %.2f)" % (b, v["ms"], v["ratio_to_gene_stats"]) for b, v in r["by_groups"].items())))
    ok = all(v["n_cells_add_up"] for where in ("device_resident", "host_resident") if gb.get(where) for v in gb[where]["by_groups"].values())
    vals["GROUPS_MEASURED"] = ("One MI355X, %s cells x %d genes, %.0f stored counts per cell, medians by the library's timers (the whole call): %s. The group counts add up "
                               "to the ungrouped ones in every run: %s."
                               % ("{:,}".format(gb["cells"]).replace(",", " "), gb["G_all"], gb["nnz_per_cell"], "; ".join(rows), "yes" if ok else "NO"))
else:
    vals["GROUPS_MEASURED"] = "**Not measured yet**: `profiles/group_stats_bench.json` (written by `tools/group_stats_bench.py` on an MI355X) is not in the tree."
rb = line("ranksum_bench.json")      # tools/ranksum_bench.py
if rb:
    rows = []
    for where in ("device_resident", "host_resident"):
        r = rb.get(where)
        if r:
            rows.append("%s `rank_sums` %.0f ms (spread, (max - min) / median, %.1f %% over %d calls) in %d gene block%s%s: count sweep %.0f ms, fill sweeps %.0f ms, "
                        "sort and rank %.0f ms; `gene_stats_by_group` beside it %.1f ms (spread %.1f %%), ratio %.1f; %s list entries, %s of them on the radix path: "
                        "the byte bound of the lists is %.1f ms"
                        % (where.replace("_", "-"), r["ms"], 100.0 * r["spread"], len(r["ms_all"]), r["gene_blocks"], "" if r["gene_blocks"] == 1 else "s",
                           ", %d slabs per sweep" % r["slabs"] if r["slabs"] > 1 else "", r["count_ms"], r["fill_ms"], r["sort_ms"], r["gene_stats_grouped_ms"],
                           100.0 * r["gene_stats_grouped_spread"], r["ratio_to_gene_stats_grouped"], "{:,}".format(r["entries"]).replace(",", " "),
                           "{:,}".format(r["entries_on_the_radix_path"]).replace(",", " "), r["bound_ms_list_bytes"]))
    ok = all(rb[w]["n_pos_equals_n_cells"] and rb[w]["rank_sums_add_up"] and rb[w].get("same_integers_as_the_first_residence", True)
             for w in ("device_resident", "host_resident") if rb.get(w))
    cpu = rb.get("cpu_scipy_spec")
    vals["RANKSUM_MEASURED"] = ("**Measured** (`profiles/ranksum_bench.json`, one MI355X, %s cells x %d genes, %.0f stored counts per cell, B = %d, medians by the library's "
                                "timers): %s. The positive counts equal `gene_stats_by_group`'s, the rank sums add up to N(N + 1) and both residences give the same "
                                "integers: %s. CPU yardstick, as measured and not extrapolated: %s."
                                % ("{:,}".format(rb["cells"]).replace(",", " "), rb["G_all"], rb["nnz_per_cell"], rb["groups"], "; ".join(rows), "yes" if ok else "NO",
                                   "the scipy spec takes %.0f s on %s cells x %d genes" % (cpu["seconds"], "{:,}".format(cpu["cells"]).replace(",", " "), cpu["genes"])
                                   if cpu else "scipy did not import"))
    try:      # the kernel trace of the device-resident call (rocprofv3 --kernel-trace --stats, a run of its own)
        import csv
        tot = {}
        for row in csv.DictReader(open(os.path.join(P, "ranksum_kernel_stats.csv"))):
            name = row["Name"].replace("void ", "").replace("hmx::", "").split("(")[0]
            tot[name] = tot.get(name, 0.0) + float(row["TotalDurationNs"]) / 1e6
        vals["RANKSUM_FILL_KERNEL_MS"] = fmt(sum(v for k, v in tot.items() if k.startswith("k_rank_sweep<") and k.endswith(", true>")))
        vals["RANKSUM_COUNT_KERNEL_MS"] = fmt(sum(v for k, v in tot.items() if k.startswith("k_rank_sweep<") and k.endswith(", false>")))
        vals["RANKSUM_SORT_KERNEL_MS"] = fmt(tot.get("k_rank_sort", 0.0))
        vals["RANKSUM_GROUPED_KERNEL_MS"] = fmt(sum(v for k, v in tot.items() if k.startswith("k_gene_stats_grouped")))
    except Exception:
        missing.append("ranksum_kernel_stats.csv")
else:
    vals["RANKSUM_MEASURED"] = "**Not measured yet**: `profiles/ranksum_bench.json` (written by `tools/ranksum_bench.py` on an MI355X) is not in the tree."
gr = line("graph_bench.json")      # tools/graph_bench.py
if gr:
    rows = []
    for r in gr["runs"]:
        rows.append("`n_neighbors` = %d: kNN %.0f ms, graph stage %.1f ms (spread %.1f %% over %d calls) = %.1f %% of the kNN in front of it, %s entries, largest "
                    "in-degree %d; byte bound %.2f ms, so the stage runs at %.1f %% of it; components within labels %.1f ms (%d components, %d within labels, graph "
                    "connectivity %.4f); the same bits in every call: %s"
                    % (r["n_neighbors"], r["knn_ms"], r["graph_ms"], 100.0 * r["graph_spread"], len(r["graph_ms_all"]), 100.0 * r["graph_share_of_knn"],
                       "{:,}".format(r["entries"]).replace(",", " "), r["max_in_degree"], r["bound_ms_bytes"], 100.0 * r["share_of_bound"],
                       r["components_within_labels_ms"], r["components"], r["components_within_labels"], r["graph_connectivity"],
                       "yes" if r["same_bits_every_call"] else "NO"))
    vals["GRAPH_MEASURED"] = ("**Measured** (`profiles/graph_bench.json`, one MI355X, %s cells x %d PCs, float32 on the host, medians by the library's timers): %s."
                              % ("{:,}".format(gr["cells"]).replace(",", " "), gr["d"], "; ".join(rows)))
    try:      # the kernel table of the n_neighbors = 15 calls (rocprofv3 --kernel-trace --stats, a run of its own)
        import csv
        ks = []
        for row in csv.DictReader(open(os.path.join(P, "graph_kernel_stats.csv"))):
            name = row["Name"].replace("void ", "").replace("hmx::", "").split("(")[0]
            if name.startswith(("k_graph_", "k_smooth_knn", "k_scan_", "k_cc_")):
                ks.append((float(row["AverageNs"]) / 1e6, int(row["Calls"]), name))
        vals["GRAPH_KERNELS"] = "; ".join("`%s` %.3f ms x %d" % (n, ms, c) for ms, c, n in sorted(ks, reverse=True))
    except Exception:
        missing.append("graph_kernel_stats.csv")
else:
    vals["GRAPH_MEASURED"] = "**Not measured yet**: `profiles/graph_bench.json` (written by `tools/graph_bench.py` on an MI355X) is not in the tree."
sn = line("snn_bench.json")      # tools/snn_bench.py
if sn:
    cpu = (" scipy's `A @ A.T` with the same pruning on that machine's CPU (one thread): %.1f s, %.0f times the SNN stage; its result equals the library's: %s."
           % (sn["cpu_scipy_ms"] / 1e3, sn["cpu_scipy_ms"] / sn["snn_ms"], "yes" if sn["equals_scipy"] else "NO")) if "cpu_scipy_ms" in sn else ""
    vals["SNN_MEASURED"] = ("**Measured** (`profiles/snn_bench.json`, one MI355X, %s cells x %d PCs, float32 on the host, k = %d, prune = %.4f so s_min = %d, medians by the "
                            "library's timers): kNN %.0f ms, SNN stage %.1f ms (spread %.1f %% over %d calls) = %.1f %% of the kNN in front of it, CSR copy of %.0f MB "
                            "included; %s entries = %.1f per row = %.2f N k against the first capacity of 6 N k (retried: %s); Σ C_i = %s candidates (%.0f per row, at most %d), "
                            "%d rows on the long path, largest in-degree %d; the same bits in every call: %s.%s"
                            % ("{:,}".format(sn["cells"]).replace(",", " "), sn["d"], sn["k"], sn["prune"], sn["s_min"], sn["knn_ms"], sn["snn_ms"], 100.0 * sn["snn_spread"],
                               len(sn["snn_ms_all"]), 100.0 * sn["snn_share_of_knn"], sn["csr_copy_bytes"] / 1e6, "{:,}".format(sn["entries"]).replace(",", " "),
                               sn["entries_per_row"], sn["entries"] / (float(sn["cells"]) * sn["k"]), "yes" if sn["retried"] else "no",
                               "{:,}".format(sn["sum_candidates"]).replace(",", " "), sn["sum_candidates"] / float(sn["cells"]), sn["max_candidates"], sn["long_rows"],
                               sn["max_in_degree"], "yes" if sn["same_bits_every_call"] else "NO", cpu))
    try:      # the kernel table of two calls (rocprofv3 --kernel-trace --stats, a run of its own)
        import csv
        ks = []
        for row in csv.DictReader(open(os.path.join(P, "snn_kernel_stats.csv"))):
            name = row["Name"].replace("void ", "").replace("hmx::", "").split("(")[0]
            if name.startswith(("k_snn_", "k_graph_", "k_scan_", "k_knn")):
                ks.append((float(row["AverageNs"]) / 1e6, int(row["Calls"]), name))
        vals["SNN_KERNELS"] = "; ".join("`%s` %.3f ms x %d" % (n, ms, c) for ms, c, n in sorted(ks, reverse=True))
    except Exception:
        vals["SNN_KERNELS"] = "not traced yet (`profiles/snn_kernel_stats.csv` is not in the tree)"
        missing.append("snn_kernel_stats.csv")
else:
    vals["SNN_MEASURED"] = "**Not measured yet**: `profiles/snn_bench.json` (written by `tools/snn_bench.py` on an MI355X) is not in the tree."
    vals["SNN_KERNELS"] = "not traced yet"
lv = line("louvain_bench.json")      # tools/louvain_bench.py
if lv:
    cpu = (" networkx's `louvain_communities` on that machine's CPU (one thread) on the same graph: %.1f s, %.0f times as long, %d clusters at Q %.5f."
           % (lv["cpu_networkx_ms"] / 1e3, lv["cpu_networkx_ms"] / lv["louvain_ms"], lv["cpu_clusters"], lv["cpu_modularity"])) if "cpu_networkx_ms" in lv \
        else " No one-thread CPU Louvain beside it: %s." % lv.get("cpu_skipped", "not run")
    vals["LOUVAIN_MEASURED"] = ("**Measured** (`profiles/louvain_bench.json`, one MI355X, the SNN graph of %s cells x %d PCs at k = %d, %s entries, resolution %.1f, "
                                "`\"timer:louvain\"` alone, median of %d calls): %.0f ms (spread %.1f %%) for %d levels and %d sweeps: %s clusters per level, Q %s, "
                                "%d clusters at Q %.5f returned (level %d); %d rows on the long path at level 0; the same bits in every call: %s. The CSR crosses the "
                                "host: %.0f MB in, %.0f ms at 50 GB/s, which a graph kept in HBM after `hmx_snn_graph` would save.%s"
                                % ("{:,}".format(lv["cells"]).replace(",", " "), lv["d"], lv["k"], "{:,}".format(lv["entries"]).replace(",", " "), lv["resolution"],
                                   len(lv["louvain_ms_all"]), lv["louvain_ms"], 100.0 * lv["louvain_spread"], lv["levels"], lv["sweeps"],
                                   " → ".join(str(c) for c in lv["level_clusters"]), " → ".join("%.4f" % q for q in lv["level_modularity"]), lv["clusters"],
                                   lv["modularity"], lv["best_level"], lv["long_rows"], "yes" if lv["same_bits_every_call"] else "NO", lv["csr_bytes"] / 1e6,
                                   lv["upload_ms_at_50GBs"], cpu))
    sm = line("louvain_bench_100k.json")      # the same tool at --cells 100000, where networkx holds the graph
    if sm and "cpu_networkx_ms" in sm:
        vals["LOUVAIN_MEASURED"] += (" At %s cells (`profiles/louvain_bench_100k.json`, %s entries) the library takes %.0f ms for %d clusters at Q %.5f; networkx's "
                                     "`louvain_communities(seed=0)` on one thread of that machine's CPU takes %.1f s, %.0f times as long, for %d clusters at Q %.5f."
                                     % ("{:,}".format(sm["cells"]).replace(",", " "), "{:,}".format(sm["entries"]).replace(",", " "), sm["louvain_ms"], sm["clusters"],
                                        sm["modularity"], sm["cpu_networkx_ms"] / 1e3, sm["cpu_networkx_ms"] / sm["louvain_ms"], sm["cpu_clusters"], sm["cpu_modularity"]))
else:
    vals["LOUVAIN_MEASURED"] = "**Not measured yet**: `profiles/louvain_bench.json` (written by `tools/louvain_bench.py` on an MI355X) is not in the tree."
um = line("umap_bench.json")      # tools/umap_bench.py
if um:
    def um_text(u):
        return ("%s cells x %d PCs, `neighbors(n_neighbors=%d)`: %s entries, longest row %d, %d epochs from the PCA start, `\"timer:umap\"` alone, median of %d calls: "
                "**%.0f ms** (spread %.1f %%), of which %.1f ms (%.0f %%) are the upload of the CSR (%.0f MB) and the checks in front of the epochs (a call that asks for "
                "no epoch); %.3f ms per epoch = %.0f epochs/s; %s firings per epoch gather %.0f MB of positions (%.2f TB/s) beside %.0f MB streamed (%.2f TB/s); %d rows on "
                "the long path; the same bits in every call: %s; trustworthiness (k = 15) of %d sampled cells %.4f (the PCA start: %.4f), kNN purity by cell type %.4f"
                % ("{:,}".format(u["cells"]).replace(",", " "), u["d"], u["n_neighbors"], "{:,}".format(u["entries"]).replace(",", " "), u["longest_row"], u["epochs"],
                   len(u["umap_ms_all"]), u["umap_ms"], 100.0 * u["umap_spread"], u["front_ms"], 100.0 * u["front_share"], u["csr_bytes"] / 1e6, u["epoch_ms"],
                   u["epochs_per_s"], "{:,}".format(int(u["firings_per_epoch"])).replace(",", " "), u["gather_bytes_per_epoch"] / 1e6, u["gather_TBps"],
                   u["stream_bytes_per_epoch"] / 1e6, u["stream_TBps"], u["long_rows"], "yes" if u["same_bits_every_call"] else "NO", u["sample"],
                   u["trustworthiness"], u["trustworthiness_of_start"], u["knn_purity"]))
    vals["UMAP_MEASURED"] = ("**Measured** (`profiles/umap_bench.json`, one MI355X): " + um_text(um) + ". Against the machine: the gathers are 64-byte lines of an "
                             "8 MB array that stays in cache, so %.2f TB/s of useful bytes is %.1f TB/s of lines, against about 8.6 TB/s measured for random rows out "
                             "of the Infinity Cache and 6.3 TB/s achievable from HBM for the streamed part: the epoch is bound by the latency of its dependent loads, "
                             "not by either rate. No CPU UMAP was raced against it: umap-learn was not installed on that machine, and the pure-Python loop of the "
                             "spec is no yardstick." % (um["gather_TBps"], um["gather_TBps"] * 64.0 / 8.0))
    sm = line("umap_bench_100k.json")
    if sm:
        vals["UMAP_MEASURED"] += " At " + um_text(sm) + " (`profiles/umap_bench_100k.json`)."
    try:      # the kernel table of one call at 1M cells (rocprofv3 --kernel-trace --stats, a run of its own)
        import csv
        ks = []
        for row in csv.DictReader(open(os.path.join(P, "umap_kernel_stats.csv"))):
            name = row["Name"].replace("void ", "").replace("hmx::", "").split("(")[0]
            if name.startswith(("k_um_", "k_lv_check", "k_cc_check")):
                ks.append((float(row["AverageNs"]) / 1e6, int(row["Calls"]), name))
        vals["UMAP_MEASURED"] += " Per kernel (`profiles/umap_kernel_stats.csv`, two calls, one of them for no epoch): " + "; ".join("`%s` %.3f ms x %d" % (n, ms, c) for ms, c, n in sorted(ks, reverse=True)) + "."
    except Exception:
        missing.append("umap_kernel_stats.csv")
else:
    vals["UMAP_MEASURED"] = "**Not measured yet**: `profiles/umap_bench.json` (written by `tools/umap_bench.py` on an MI355X) is not in the tree."
ldn = line("leiden_bench.json")      # tools/leiden_bench.py
if ldn:
    def ld_text(u):
        return ("the SNN graph of %s cells x %d PCs at k = %d, %s entries, resolution %.1f, median of %d calls: `\"timer:leiden\"` **%.0f ms** (spread %.1f %%) -- local "
                "moves and the levels' records %.0f ms, refinement with its `cut` %.0f ms, aggregation %.0f ms -- for %d levels, %d sweeps of moves and %d of "
                "refinement: %s clusters over %s nodes per level, %d clusters at Q %.5f, converged: %s, %d components inside them; `\"timer:louvain\"` on the same "
                "handle and graph %.0f ms (spread %.1f %%), %d clusters at Q %.5f with %d components inside them; %d rows on the long path; the same bits in every call: %s"
                % ("{:,}".format(u["cells"]).replace(",", " "), u["d"], u["k"], "{:,}".format(u["entries"]).replace(",", " "), u["resolution"], len(u["leiden_ms_all"]),
                   u["leiden_ms"], 100.0 * u["leiden_spread"], u["leiden_moves_ms"], u["leiden_refine_ms"], u["leiden_aggregate_ms"], u["levels"], u["sweeps"],
                   u["refine_sweeps"], " → ".join(str(c) for c in u["level_clusters"]), " → ".join(str(c) for c in u["level_nodes"]), u["clusters"], u["modularity"],
                   "yes" if u["converged"] else "NO", u["components_within_clusters"], u["louvain_ms"], 100.0 * u["louvain_spread"], u["louvain_clusters"],
                   u["louvain_modularity"], u["louvain_components_within_clusters"], u["long_rows"], "yes" if u["same_bits_every_call"] else "NO"))
    vals["LEIDEN_MEASURED"] = ("**Measured** (`profiles/leiden_bench.json`, one MI355X, `tools/leiden_bench.py`; both timers include the upload of the CSR; `cut` is the "
                               "recomputed form and interleaves with the refinement's decisions on the stream, so the two are one figure): " + ld_text(ldn) + ".")
    sm = line("leiden_bench_100k.json")
    if sm:
        vals["LEIDEN_MEASURED"] += " At " + ld_text(sm) + " (`profiles/leiden_bench_100k.json`)."
else:
    vals["LEIDEN_MEASURED"] = ("**Nothing has been measured on a device yet**: `profiles/leiden_bench.json` (written by `tools/leiden_bench.py` on an MI355X, which times "
                               "`hmx_leiden` beside `hmx_louvain` on the same SNN graphs at 100k and 1M cells, with the phases' times) is not in the tree.")
ut = line("umap_transform_bench.json")      # tools/umap_transform_bench.py
if ut:
    def ut_text(r):
        return ("%s query cells, %d epochs: the search `\"timer:knn\"` %.0f ms; `\"timer:umap_query_weights\"` **%.2f ms** (spread %.0f %%); `\"timer:umap_transform\"` "
                "**%.2f ms** (spread %.0f %%), of which %.2f ms are the uploads (%.0f MB) and the start (a call that asks for no epoch) and **%.3f ms** the epochs' one "
                "kernel (`\"timer:umap_transform_epochs\"`, between two events; spread %.1f %%): %s firings, %.1f per cell and epoch, **%.3f ns per firing**, "
                "%.0f MB of sampled positions gathered (%.2f TB/s of useful bytes); with the lists and samples folded onto 1024 reference cells the kernel takes "
                "%.3f ms, so %.0f %% of its time goes with the gathers' misses; the same bits in every call: %s; mean |Y - Y0| %.3f"
                % ("{:,}".format(r["query"]).replace(",", " "), r["epochs"], r["knn_ms"], r["weights_ms"], 100.0 * r["weights_spread"], r["transform_ms"],
                   100.0 * r["transform_spread"], r["front_ms"], r["upload_bytes"] / 1e6, r["epochs_ms"], 100.0 * r["epochs_spread"],
                   "{:,}".format(r["fired"]).replace(",", " "), r["firings_per_cell_epoch"], r["ns_per_firing"], r["gather_bytes"] / 1e6, r["gather_TBps"],
                   r["cached_epochs_ms"], 100.0 * r["gather_share"], "yes" if r["same_bits_every_call"] else "NO", r["mean_move"]))
    big = ut["runs"][0]
    vals["UMAP_TRANSFORM_MEASURED"] = (
        "**Measured** (`profiles/umap_transform_bench.json`, one MI355X, `tools/umap_transform_bench.py`: a reference of %s cells x %d PCs laid out by `umap()`, "
        "k = %d, medians of %d calls after %d; the wall timers are a few milliseconds of copies from pageable memory and spread accordingly, the kernel's "
        "time does not): " % ("{:,}".format(ut["reference"]).replace(",", " "), ut["d"], ut["k"], ut["repeats"], ut["warmup"])
        + "; ".join(ut_text(r) for r in ut["runs"]) + ". "
        + ("`hmx_umap_layout` spends %.3f ns per firing at 10\u2076 cells (`profiles/umap_bench.json`: an epoch's time over its firings), %.1f times as much: there a "
           "firing also gathers its attraction's other end, walks the CSR and writes a snapshot per epoch. " % (ut["layout_ns_per_firing"], ut["layout_ns_per_firing"] / big["ns_per_firing"])
           if ut.get("layout_ns_per_firing") else "")
        + "**What bounds the kernel: the sample gathers, not the dependent chain.** At %s query cells %s firings x %d samples are %.0f million 8-byte reads, each its "
          "own 64-byte line of an 8 MB array: %.1f TB/s of lines, against about 8.6 TB/s measured for random rows out of the Infinity Cache (\u00a76m). The per-epoch "
          "chain (`log2f`/`exp2f`, the butterfly, the fp64 firing test) is what is left when every gather hits: %.0f %% of the time. With few cells (10\u2074: 2 500 "
          "waves on 1 024 SIMDs) the chain's share grows, since there are too few waves to hide either latency."
          % ("{:,}".format(big["query"]).replace(",", " "), "{:,}".format(big["fired"]).replace(",", " "), big["negative_sample_rate"],
             big["fired"] * big["negative_sample_rate"] / 1e6, big["fired"] * big["negative_sample_rate"] * 64.0 / big["epochs_ms"] / 1e9,
             100.0 * (1.0 - big["gather_share"])))
else:
    vals["UMAP_TRANSFORM_MEASURED"] = ("**Not measured yet**: `profiles/umap_transform_bench.json` (written by `tools/umap_transform_bench.py` on an MI355X) is not "
                                       "in the tree.")
db = line("doublets_bench.json")      # tools/doublets_bench.py
if db:
    def db_text(r):
        return ("%s observed cells (%s synthetic, %.0f stored counts per cell): `\"timer:simulate_doublets\"` **%.1f ms** (spread %.0f %%), %.0f ns per synthetic cell; "
                "the parents' rows read twice are %.1f GB, %.2f ms at %.1f TB/s if all of it came from HBM: **%.1f times the bound**; the same bits in every call: %s"
                % ("{:,}".format(r["cells"]).replace(",", " "), "{:,}".format(r["n_sim"]).replace(",", " "), r["nnz_per_cell"], r["timer_ms_median"],
                   100.0 * r["timer_spread"], r["ns_per_synthetic_cell"], r["bytes_parents_read_twice"] / 1e9, r["bound_ms_parents_twice_from_hbm"],
                   db["hbm_bytes_per_s_assumed"] / 1e12, r["ratio_to_bound"], "yes" if r["same_bits_every_call"] else "NO"))
    vals["DOUBLETS_MEASURED"] = ("**Measured** (`profiles/doublets_bench.json`, one MI355X, `tools/doublets_bench.py`: G_all = %d, G = %d, d = %d, r = %g, the matrix "
                                 "device-resident, medians of %d calls after %d; the timer includes the uploads of the tables and the pairs and the download of the "
                                 "PCs): " % (db["G_all"], db["G"], db["d"], db["ratio"], db["repeats"], db["warmup"]) + "; ".join(db_text(r) for r in db["runs"]) + ".")
    nb = db.get("neighbors")
    if nb:
        vals["DOUBLETS_MEASURED"] += (" `hmx_doublet_neighbors` at %s + %s rows x %d PCs, k_adj = %d: the search `\"timer:knn\"` %.0f ms, the counts behind it "
                                      "`\"timer:doublet_neighbors\"` %.2f ms." % ("{:,}".format(nb["n_obs"]).replace(",", " "), "{:,}".format(nb["n_sim"]).replace(",", " "),
                                                                                     nb["d"], nb["k_adj"], nb["knn_ms_median"], nb["count_ms"]))
else:
    vals["DOUBLETS_MEASURED"] = ("**Not measured yet**: `profiles/doublets_bench.json` (written by `tools/doublets_bench.py` on an MI355X: the time of "
                                 "`hmx_simulate_doublets` at 10\u2075 and 10\u2076 observed cells beside the bound of the parents' rows read twice from HBM) is not in the tree.")
parts = sorted(f for f in os.listdir(os.path.join(ROOT, "docs", "design_parts")) if f.endswith(".md"))
out = io.StringIO()
for f in parts:
    out.write(open(os.path.join(ROOT, "docs", "design_parts", f)).read().rstrip("\n") + "\n\n")
text = out.getvalue()
import re
for k in sorted(set(re.findall(r"@@([A-Z0-9_]+)@@", text))):
    if k in vals:
        text = text.replace("@@%s@@" % k, vals[k])
    else:
        text = text.replace("@@%s@@" % k, "n/a")
        missing.append("placeholder " + k)
open(os.path.join(ROOT, "DESIGN.md"), "w").write(text.rstrip("\n") + "\n")
# README.md from docs/readme_template.md: the same placeholders
rt = open(os.path.join(ROOT, "docs", "readme_template.md")).read()
for k in sorted(set(re.findall(r"@@([A-Z0-9_]+)@@", rt))):
    rt = rt.replace("@@%s@@" % k, vals.get(k, "n/a"))
    if k not in vals:
        missing.append("README placeholder " + k)
open(os.path.join(ROOT, "README.md"), "w").write(rt)
print("DESIGN.md: %d bytes from %d parts; %d placeholders filled" % (len(text), len(parts), len(vals)))
if missing:
    print("MISSING:", "; ".join(missing))
