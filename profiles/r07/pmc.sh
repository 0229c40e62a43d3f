#!/bin/bash
# SQ counter passes over the bf16 probe (one group per rocprofv3 run, no trace domains); stop at the first failure
set -u
rm -rf out/pmc; mkdir -p out/pmc
i=0
for grp in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_VALU_MFMA_BUSY_CYCLES" \
           "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_ANY" \
           "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $grp --output-format csv -d out/pmc/g$i -- python tools/full_softmax_probe.py --reps 1 --tiers bf16 > out/pmc/log$i.txt 2>&1
  rc=$?; [ $rc -eq 0 ] || { tail -20 out/pmc/log$i.txt; exit $rc; }
done
python - <<'PY' > out/pmc/pmc_counters.txt
import csv, glob, collections
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("out/pmc/g*/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"]
        if "full_ce" not in k or "reduce" in k: continue
        kk = "fwd train" if ("true" in k or "Lb1" in k) else ("fwd infer" if ("false" in k or "Lb0" in k) else "dW")
        acc[kk][row["Counter_Name"]].append(float(row["Counter_Value"]))
for k in ("fwd train", "fwd infer", "dW"):
    print("bf16 %s (d = 128, configs[1]; mean over its dispatches)" % k)
    for c, v in sorted(acc[k].items()):
        print("  %-28s %18.0f  (n=%d)" % (c, sum(v) / len(v), len(v)))
PY
cat out/pmc/pmc_counters.txt
