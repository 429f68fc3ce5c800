"""Benchmark: questions/sec reweighted-decode + heads/sec IE-sweep, Llama-3-8B NQ-1000 (BASELINE.json).

Default (config 3 + 2): one step = the full Find_Best_Heads IE sweep (32 layers x
32 heads) of ONE NQ question per GPU (weak scaling; questions are dealt to ranks,
no data-path collective), plus one RCCL all-gather of the IE grids at the end of
the timed region.  The primary `value` is heads/s over all ranks; the batched
reweighted decode (questions/s, config 2) is reported next to it as `decode`.
Other BASELINE configs:  --config 1 (GPT-2-small, 8 NQ questions x 5 docs, the reference's batch-1 hooked
decode shape: drop-in on the HIP kernels vs the CPU hook path), --config 2 (decode as the primary value),
--config 4 (Qwen2-7B, TriviaQA, ideal scores, all heads, decode),
--config 5 (Llama-3-8B, 20 retrieved docs ~8k tokens, decode).

Run:  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
      (N > 1 under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`)
A plain run does what the headline figure needs and no more: set-up, W warm-up steps, K timed steps, the result line
(config 3: the IE sweep alone; configs 1, 2, 4, 5: the decode alone).  --full adds everything else the line can
carry: config 3's decode leg (config 2's workload, `decode`), the decode attention kernel's roofline launches and the
CPU baselines (`cpu_baseline`, `speedup_vs_cpu`).  --dump-outputs DIR writes what the last timed step returned to its
caller as DIR/<name>.npy (config 3: `ie`, the IE grids [questions of the step, L, H]; decode: `decode_answers`, the
generated ids [questions, new tokens]); the inputs are the same from run to run, so two builds compare output for output.
Weights are random-init of the named architecture (no checkpoint offline);
prompts are the rebuilt NQ/TriviaQA-1000 inputs through the offline BPE tokenizers
with the model family's chat template (mean ~962 tokens with the wrong answer appended).
"""
from __future__ import annotations

import argparse
import gzip
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

METRIC = "questions/sec reweighted-decode + heads/sec IE-sweep, Llama-3-8B NQ-1000"
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md, chip table)
PEAK_HBM_GBS = 8000.0          # MI355X HBM3E (MI355X_MICROARCH.md; ~6300 achievable)
PMC_FILE = os.path.join(REPO, "profiles", "attn_pmc.json")
GEMM_PMC_FILE = os.path.join(REPO, "profiles", "gemm_pmc.json")
PMC_KEYS = ("mfma_busy", "effective_clock_ghz", "valu_per_mfma", "mfma_issues_over_algorithmic", "hbm_gbs", "hbm_frac",
            "tflops", "mfma_frac_of_peak", "avg_launch_ms_under_pmc", "wait_any_frac")


def decode_attention_roofline(eng, prompts, weights16, heads, new_tokens, dev, iters=20):
    """HBM roofline of the decode attention kernel at the decode leg's own shape (outside its timed region): a
    DecodeSession is prefilled with the same prompts, then cram_attn_decode on layer 0 (its bias, head enable,
    split count and workspace) is launched `iters` times and timed with HIP events on the launch stream.
    Algorithmic bytes = the visible K and V rows (sum of the sequence lengths x Hkv x d x 2 tensors x 2 B)."""
    import torch
    from cram_amd import ops
    from cram_amd.engine import DecodeSession
    sp = eng.spec
    sess = DecodeSession(eng, prompts, weights16, heads, new_tokens)
    sess.prefill()
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(sess.B, sp.num_heads, sp.head_dim, device=dev, generator=g).to(eng.dtype)
    out = torch.empty_like(q)

    def run():
        ops.attn_decode(q, sess.k_cache[0], sess.v_cache[0], scale=eng.scale, seq_lens=sess.seq_lens,
                        bias=sess.cb.bias, enable=sess.cb.enable[0], W=sess.cb.W, num_splits=sess.splits,
                        workspace=sess.ws, out=out, shared_rows=sess.shared_read)

    for _ in range(3):
        run()
    st = torch.cuda.current_stream(dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    for _ in range(iters):
        run()
    e.record(st)
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / iters
    # visible K/V rows; the batch's shared opening (whole 32-key blocks, read from cache row 0) counted once
    sh = sess.shared_read // 32 * 32
    kv_bytes = float(sum(sess.lens) - (sess.B - 1) * sh) * sp.num_kv_heads * sp.head_dim * 2 * 2
    ach = kv_bytes / (ms * 1e-3) / 1e9
    G = sp.num_heads // sp.num_kv_heads
    kern = ("decode_mfma_kernel (16x16x32 matrix cores, GQA group of %d)" % G if G >= 4 and sp.head_dim == 128
            else "decode_kernel (VALU)") + (" + decode_combine_kernel (split %d)" % sess.splits if sess.splits > 1 else "")
    res = {"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
           "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": None, "kernel": kern,
           "avg_launch_ms": round(ms, 4), "bytes_per_launch": kv_bytes, "batch": sess.B, "splits": sess.splits,
           "shared_rows_read_once": sh,
           "note": "layer 0 of the decode leg's prefilled KV cache, timed apart from the decode leg"}
    del sess
    torch.cuda.empty_cache()
    return res


def decode_leg_roofline(spec, phases, dtype):
    """Roofline of the whole decode leg, from HIP events recorded inside it (engine.generate(phases=...)), summed
    over the timed repeats:
      prefill  MFMA-bound: algorithmic FLOPs of the packed prefill — per prompt of T tokens, every layer's
               projections 2 * params * T (ModelSpec.layer_flops) + causal attention 4 * d * Hq * T(T+1)/2, and the
               lm_head of the last row 2 * D * V — over the prefill's time, against the dense bf16 peak; the rows of
               the batch's shared prefix (DecodeSession.shared_prefix, computed once) are counted once;
      steps    HBM-bound: per greedy step, every weight once (L layers' projections + lm_head, the embedding is a
               B-row gather) + every row's visible K and V (L * Hkv * d * 2 tensors * 2 B per key, the keys growing
               by one per step; the batch's shared opening, read from one cache row, once) over the steps' time,
               against 8 TB/s (6.3 achievable)."""
    import torch  # noqa: F401
    L, D, V = spec.num_layers, spec.hidden, spec.vocab
    esz = 2
    p_layer = spec.hidden * (spec.q_size + 2 * spec.kv_size) + spec.q_size * spec.hidden + 3 * spec.hidden * spec.intermediate
    w_bytes = (L * p_layer + V * D) * esz
    kv_per_key = L * spec.num_kv_heads * spec.head_dim * 2 * esz
    pf_flops = pf_ms = st_bytes = st_ms = cap_ms = 0.0
    n_steps = 0
    for ph in phases:
        lens = ph["lens"]
        p = ph.get("prefix", 0)
        att = lambda T: L * 4.0 * spec.head_dim * spec.num_heads * T * (T + 1) / 2
        if p:
            pf_flops += L * spec.layer_flops(p) + att(p)
        for T in lens:
            pf_flops += L * spec.layer_flops(T - p) + att(T) - att(p) + 2.0 * D * V
        pf_ms += ph["t0"].elapsed_time(ph["prefill"])
        cap_ms += ph["prefill"].elapsed_time(ph["capture"])
        st_ms += ph["capture"].elapsed_time(ph["steps"])
        shr = ph.get("shared_read", 0) * (len(lens) - 1)       # the shared opening's rows, read once per step
        for t in range(1, ph["n_steps"] + 1):
            st_bytes += w_bytes + kv_per_key * (sum(T + t for T in lens) - shr)
        n_steps += ph["n_steps"]
    pf = pf_flops / (pf_ms * 1e-3) / 1e12
    bw = st_bytes / (st_ms * 1e-3) / 1e9
    return {"prefill": {"bound": "mfma", "achieved": round(pf, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(pf / PEAK_BF16_TFLOPS, 4), "ms": round(pf_ms / len(phases), 2),
                        "flops": pf_flops / len(phases)},
            "steps": {"bound": "hbm", "achieved": round(bw, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                      "frac": round(bw / PEAK_HBM_GBS, 4), "ms": round(st_ms / len(phases), 2),
                      "ms_per_step": round(st_ms / max(1, n_steps), 3), "bytes_per_step": st_bytes / max(1, n_steps),
                      "weight_bytes_per_step": w_bytes},
            "graph_capture_ms": round(cap_ms / len(phases), 2),
            "note": "HIP events on the launch stream inside engine.generate: each rate is the timed batches' summed "
                    "work over their summed time; the ms fields are means per decode batch (ms_per_step per step)"}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


DUMP_LIMIT = 64 * 10**6       # bytes of --dump-outputs in all


def dump_outputs(path, arrays, limit=DUMP_LIMIT):
    """--dump-outputs: every array of {name: ndarray} as path/<name>.npy, float32 (float64 arrays stay float64).  The
    files hold at most `limit` bytes in all: a larger set is cut to a fixed sample, the same elements of every array's
    flattened values in every run (numpy default_rng(0), sorted indices), each array keeping its share of the bytes."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
              for k, a in arrays.items()}
    total = sum(a.nbytes + 128 for a in arrays.values())          # + the .npy header
    for name, a in arrays.items():
        if total > limit:
            keep = max(1, int(a.size * limit / total) - 128 // a.itemsize)
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def load_dataset(name):
    with gzip.open(os.path.join(REPO, "data", f"{name}_1000.json.gz"), "rt", encoding="utf-8") as f:
        return json.load(f)


def long_context_paras(data, i, n_docs=20, seed=0):
    """Config 5: 20 retrieved 'documents' per question, each 2-4 concatenated pool passages
    (numpy default_rng(seed + i) over the rebuilt passages), the question's fake passage at a seeded
    position (score 0.1), the others 1.0."""
    import numpy as np
    rng = np.random.default_rng(seed + i)
    rec = data[i]
    pool = [p for j, r in enumerate(data) if j != i for p in r["reranked_dense_ctxs"]]
    docs = list(rec["reranked_dense_ctxs"])
    while len(docs) < n_docs - 1:
        k = int(rng.integers(2, 5))
        docs.append(" ".join(pool[int(x)].strip() for x in rng.integers(0, len(pool), k)))
    pos = int(rng.integers(0, n_docs))
    paras = docs[:pos] + list(rec["ori_fake"]) + docs[pos:]
    scores = [1.0] * pos + [0.1] + [1.0] * (n_docs - 1 - pos)
    return paras[:n_docs], scores[:n_docs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=3, choices=[1, 2, 3, 4, 5])
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure as well: config 3's decode leg, the decode attention "
                         "kernel's roofline launches, the CPU baselines (a plain run times the headline workload only)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    # max rows per decode batch.  Round 6: NQ-1000 on one GPU in ONE batch of 1000 rows (KV cache ~180 GB of the 288
    # GB: --kv-frac 0.68): every decode step's 15 GB weight read and its projections serve all 1000 rows, 34.2 ms per
    # step against 2 x 18.8 for two batches of 500 -- 81.8 vs 79.5 questions/s on one box (profiles/r06/decode_b*.json;
    # round 3 moved 256 -> 512 rows: 72.4 vs 67.9)
    ap.add_argument("--decode-batch", type=int, default=1024)
    ap.add_argument("--kv-frac", type=float, default=0.68,
                    help="fraction of HBM the decode KV cache may take (rows per batch = this / bytes per row)")
    ap.add_argument("--decode-tokens", type=int, default=100, help="new tokens per question (re_weighting.py:127)")
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--scores", default="ideal", choices=["ideal", "gpt"],
                    help="decode scores: ideal [0.1,1,1,1,1] or the NQ GPT truthful scores (RAG_test.py:89-105)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prefix-skip", action="store_true", help="recompute rows before the first biased key (A/B)")
    ap.add_argument("--position-sweep", action="store_true",
                    help="config 3 as casual_tracing_per_head_with_position (find_best_heads.py:61-110): each question "
                         "swept with the fake passage at positions 0..4 among the retrieved ones (5 x L x H units)")
    ap.add_argument("--cpu-units", type=int, default=64,
                    help="IE units of the CPU baseline sample (>= 1; BASELINE.md: 1 question x 2 layers x 32 heads)")
    ap.add_argument("--cpu-decode-questions", type=int, default=2,
                    help="questions of the CPU decode baseline's sample (BASELINE.md: 2 NQ questions)")
    ap.add_argument("--cpu-decode-steps", type=int, default=8,
                    help="decode steps of the CPU decode baseline's sample (0 = skip it); extrapolated to --decode-tokens")
    ap.add_argument("--cpu-decode-layers", type=int, default=-1,
                    help="decoder layers the CPU decode sample runs, scaled to all (0 = all; -1 = 2 for prompts over "
                         "4096 tokens, else all)")
    ap.add_argument("--decode-questions", type=int, default=0,
                    help="questions decoded once across the ranks (default: the whole 1000-question set; config 5: "
                         "one KV-budget batch per GPU)")
    ap.add_argument("--blas", default="hipblaslt", choices=["hipblas", "hipblaslt"])
    ap.add_argument("--dist-backend", default=None, help="nccl (RCCL, default on GPU) or gloo (rehearsal)")
    ap.add_argument("--model", default=None, choices=["llama3-8b", "qwen2-7b", "llama2-13b"],
                    help="override the config's model: llama2-13b = the reference's default model (fp16, MHA)")
    ap.add_argument("--expandable-segments", action="store_true",
                    help="PYTORCH_HIP_ALLOC_CONF=expandable_segments:True (A/B of the caching allocator's segments)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        # a plain run: the headline figure's workload only (config 3: the sweep; the others: the decode)
        args.no_cpu_baseline = True
        args.no_decode = args.no_decode or args.config == 3
    if args.expandable_segments:
        os.environ["PYTORCH_HIP_ALLOC_CONF"] = "expandable_segments:True"      # before torch initialises HIP

    import torch
    from cram_amd import dist as cdist
    from cram_amd import ops, scores, spans, sweep
    from cram_amd.engine import CrAMEngine, ModelSpec, configure_blas

    if args.config == 1:
        return run_config1(args)
    rank, world, local = cdist.init(args.dist_backend)
    if world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}; using WORLD_SIZE")
    dev = torch.device("cuda", local % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(dev)
    from cram_amd import build as _b
    if rank == 0 and _b.needs_build():
        _b.build()
    if world > 1:
        torch.distributed.barrier()
    configure_blas(args.blas)

    model = args.model or ("qwen2-7b" if args.config == 4 else "llama3-8b")
    spec = {"qwen2-7b": ModelSpec.qwen2_7b, "llama3-8b": ModelSpec.llama3_8b, "llama2-13b": ModelSpec.llama2_13b}[model]()
    # torch_dtype="auto" of the real checkpoints: bf16 for Llama-3 / Qwen2, fp16 for Llama-2
    mdtype = torch.float16 if model == "llama2-13b" else torch.bfloat16
    t0 = time.time()
    eng = CrAMEngine.random(spec, dev, seed=1234, rope_theta={"qwen2-7b": 1e6, "llama3-8b": 500000.0,
                                                               "llama2-13b": 10000.0}[model], dtype=mdtype)
    torch.cuda.synchronize()
    log(f"[rank {rank}] random-init {model} ({mdtype}) in {time.time() - t0:.1f}s")

    from transformers import AutoTokenizer
    # no Llama-2 tokenizer offline: its prompts use the Llama-3 BPE with the reference's raw Llama-2 template
    tok = AutoTokenizer.from_pretrained(os.path.join(REPO, "data", "tok_qwen" if model == "qwen2-7b" else "tok_llama3"))
    name = {"qwen2-7b": "Qwen2-7B-Instruct", "llama3-8b": "Meta-Llama-3-8B-Instruct",
            "llama2-13b": "Llama-2-13b-chat-hf"}[model]
    dsname = "trivia" if args.config == 4 else "nq"
    data = load_dataset(dsname)
    L, H = spec.num_layers, spec.num_heads
    result = {"metric": METRIC, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
              "higher_is_better": True, "vs_baseline": None, "dtype": "fp16" if mdtype == torch.float16 else "bf16"}

    # ------------------------------------------------------------------ IE sweep (config 3)
    ie = None
    if args.config == 3:
        n_w, n_t = args.warmup * world, args.steps * world
        # weak scaling with equal per-GPU work at every N: questions are taken in order of closeness to the
        # mean prompt length (characters of question + passages + wrong answer); the warm-up and the timed set
        # (steps x N questions) each go through the product's sharded sweep (cram_amd.dist.sweep_sharded: LPT of
        # whole questions over the ranks by token count, one RCCL all-gather of the IE rows at the end)
        clen = [len(r["question"]) + sum(len(p) for p in r["ori_fake"] + r["reranked_dense_ctxs"])
                + len(r["wrong_answer"]) for r in data]
        mean_c = sum(clen) / len(clen)
        pool = sorted(range(len(data)), key=lambda i: (abs(clen[i] - mean_c), i))
        work = []
        from cram_amd import heads as Hd
        positions = range(5) if args.position_sweep else (None,)
        for s in range(n_w + n_t):
            qi = pool[s % len(pool)]
            rec = data[qi]
            ans = tok([rec["wrong_answer"]], return_tensors="pt")["input_ids"][0, 1:]
            for pos in positions:
                # the plain sweep's contexts (find_best_heads.py:41-48) or the fake passage at `pos` (:83-99)
                ctx, sc = (Hd.position_contexts(rec, pos) if pos is not None
                           else (rec["ori_fake"] + rec["reranked_dense_ctxs"], [0, 1, 1, 1, 1]))
                _, enc, w, _ = spans.encode(tok, name, rec["question"], ctx, sc, rec["wrong_answer"])
                work.append((qi, enc["input_ids"][0].to(dev), w[0], ans.to(dev)))
        n_w, n_t = n_w * len(positions), n_t * len(positions)        # work items: (question, position)
        torch.cuda.synchronize()
        mine = []

        def run_set(items, timed):
            def fn(i, layers):
                qi, ids, w, ans = items[i]
                out = sweep.ie_question(eng, ids, w, ans, layers=layers, skip_prefix=not args.no_prefix_skip)
                if timed:
                    mine.append((ids.numel(), ans.numel(), w, layers))
                log(f"[rank {rank}] {'step' if timed else 'warmup'} question {qi}: {len(layers)} layers enqueued "
                    f"({time.perf_counter() - t_start:.1f}s)")
                return out
            return cdist.sweep_sharded(fn, len(items), [x[1].numel() for x in items], L, H, dev)

        t_start = time.perf_counter()
        if n_w:
            run_set(work[:n_w], False)
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()
        ops.TIMER.reset()
        ops.TIMER.enabled = True
        t_start = time.perf_counter()
        full = run_set(work[n_w:], True)                     # sweep + the RCCL all-gather of the IE grid
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        elapsed = time.perf_counter() - t_start
        ops.TIMER.enabled = False
        flops = flops_ex = 0.0
        base_variant = not sweep.row_exact(eng)
        for T, n_ans, w, layers in mine:
            p0 = int((w.view(-1) != 1).nonzero()[0, 0]) if bool((w != 1).any()) else T
            p0 = 0 if args.no_prefix_skip else p0
            # algorithmic (SURVEY §8(d) with the prefix skip: 32 variants, answer-row q in the last layer) and what
            # the sweep executes (+ the un-perturbed variant of the default mode, the GEMMs' pad rows)
            flops += sweep.sweep_flops(spec, T, n_ans, p0, layers)
            flops_ex += sweep.sweep_flops_executed(spec, T, n_ans, p0, layers, base_variant=base_variant,
                                                   group=sweep.SWEEP_GROUP)
        ksum = ops.TIMER.summary()
        kt = ksum.get("cram_prefill", None)
        # the projections: cram_gemm (gemm_w4_kernel, every epilogue), its split-K tail, and F.linear calls left
        kg = None
        for nm in ("gemm", "cram_gemm", "cram_gemm_splitk"):
            if nm in ksum:
                kg = dict(ksum[nm]) if kg is None else {k: kg[k] + ksum[nm][k] for k in ("launches", "total_ms", "flops",
                                                                                            "bytes")}
        if kg is not None:
            kg["avg_ms"] = kg["total_ms"] / kg["launches"]
            kg["cram_share"] = (ksum["cram_gemm"]["total_ms"] / kg["total_ms"]) if "cram_gemm" in ksum else 0.0
        kc = dict(ksum["cram_gemm"]) if "cram_gemm" in ksum else None
        if kc is not None:
            kc["avg_ms"] = kc["total_ms"] / kc["launches"]
        el = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        fl = torch.tensor([flops, flops_ex], device=dev, dtype=torch.float64)
        if world > 1:
            el, fl = cdist.all_reduce_host(el, "max"), cdist.all_reduce_host(fl, "sum")
        elapsed, flops_all, flops_ex_all = float(el.item()), float(fl[0].item()), float(fl[1].item())
        units = n_t * L * H
        assert tuple(full.shape) == (n_t, L, H) and torch.isfinite(full).all(), "non-finite or missing IE"
        ie = {"value": units / elapsed, "elapsed": elapsed, "flops": flops_all, "flops_executed": flops_ex_all,
              "base_variant": base_variant, "kt": kt, "kg": kg, "kc": kc,
              "mean_T": sum(x[1].numel() for x in work) / len(work), "work": work,
              "last_step": full[-world * len(positions):]}      # the IE grids of the last timed step's questions
        log(f"[rank {rank}] IE sweep: {units} units in {elapsed:.2f}s -> {ie['value']:.1f} heads/s")

    # ------------------------------------------------------------------ batched reweighted decode (configs 2, 4, 5)
    # The question set is decoded exactly once across the ranks (cram_amd.dist.decode_sharded: LPT on prompt length,
    # each rank's share in batches of at most --decode-batch rows, answers all-gathered), as RAG_test.py:64-176 answers
    # every question once: NQ-1000 / TriviaQA-1000 for configs 2-4 (strong scaling over N), config 5 one KV-budget
    # batch per GPU of long-context questions.
    decode = answers = None
    dec_cpu_input = None
    if not args.no_decode:
        if model == "qwen2-7b":
            heads, heads_desc = {}, "all heads (no Qwen2 head fixture)"
        else:
            key = "nq__llama2_13b_chat" if model == "llama2-13b" else "nq__llama3"
            heads = json.load(open(os.path.join(REPO, "data", "selected_heads.json")))[key]["heads"]
            heads_desc = f"{key} selected_heads top-{sum(len(v) for v in heads.values())}"
        if args.config == 5:
            # 20 retrieved docs (~8.3k tokens): rows per GPU from the KV budget (decode_batch, below), one batch each
            nq_dec = args.decode_questions or world * args.decode_batch
        else:
            nq_dec = args.decode_questions or len(data)
        nq_dec = min(nq_dec, len(data))
        qs, ps, ss = [], [], []
        for qi in range(nq_dec):
            rec = data[qi]
            if args.config == 5:
                paras, sc = long_context_paras(data, qi)
            elif args.scores == "gpt" and "ori_fake_truthful_scores" in rec:
                paras, sc = scores.assemble(rec)                            # normalised + re-ordered
            else:
                paras, sc = scores.assemble(rec, ideal=True, ideal_score=1)     # [0.1, 1, 1, 1, 1]
            qs.append(rec["question"])
            ps.append(paras)
            ss.append(sc)
        th = time.perf_counter()
        encs = spans.encode_batch(tok, name, qs, ps, ss)                     # host: prompts -> ids + fp16 weights
        host_ms = (time.perf_counter() - th) * 1e3
        lens = [ids.numel() for ids, _, _ in encs]
        # the static KV cache is [L][B][Hkv][S_max][d] for K and V: rows per batch = what fits in --kv-frac of HBM
        # next to the weights (16 GB + the 7.5 GB interleaved gate/up) and the packed-prefill activations (32k-row
        # chunks, a few GB) (config 5: ~1.1 GB per 8.4k-token row -> 128 rows; MHA Llama-2-13b: 0.9 GB per
        # 1.1k-token row)
        s_max = max(lens) + args.decode_tokens
        per_row = 2 * spec.num_layers * spec.num_kv_heads * s_max * spec.head_dim * 2
        cap = max(1, int(args.kv_frac * torch.cuda.get_device_properties(dev).total_memory // per_row))
        # whole 64-row groups when the budget binds: the decode step's projections run on 128-row tiles
        # (cram_gemm_small), so one row past a multiple of 128 would cost a whole extra tile (config 5: 129 -> 128)
        cap = cap // 64 * 64 if cap >= 128 else cap
        B = min(args.decode_batch, cap)
        if B < args.decode_batch:
            log(f"[rank {rank}] decode batch {args.decode_batch} -> {B} (KV cache {per_row / 2**20:.0f} MiB per row)")
        if args.config == 5 and not args.decode_questions:
            nq_dec = min(len(data), world * B)
            encs, lens = encs[:nq_dec], lens[:nq_dec]
        prompts = [ids for ids, _, _ in encs]
        ws = [w for _, w, _ in encs]
        costs = [float(n) for n in lens]
        gen_kw = dict(max_new_tokens=args.decode_tokens, eos_ids=(), use_graph=True, stop_on_eos=False)
        my_batches = cdist.decode_batches(cdist.lpt_shards(costs, world)[rank], costs, B)
        dev_prompts = {}

        def dec_fn(idx, phases=None):
            ps_ = [dev_prompts.setdefault(i, prompts[i].to(dev)) for i in idx]
            if phases is not None:
                phases.append({})
            return eng.generate(ps_, [ws[i] for i in idx], heads, phases=phases[-1] if phases is not None else None,
                                **gen_kw)

        # warm-up at the timed shape (the packed prefill's GEMM heuristics and buffers, the batch graph)
        for _ in range(max(1, args.warmup)):
            if my_batches:
                dec_fn(my_batches[0])
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
        reps = max(1, args.steps if args.config != 3 else 1)
        phases = []
        td = time.perf_counter()
        for _ in range(reps):
            answers = cdist.decode_sharded(lambda idx: dec_fn(idx, phases), nq_dec, costs, B)
        torch.cuda.synchronize()
        dt = torch.tensor([time.perf_counter() - td], device=dev, dtype=torch.float64)
        if world > 1:
            dt = cdist.all_reduce_host(dt, "max")
        assert len(answers) == nq_dec and all(len(a) == args.decode_tokens for a in answers), "missing answers"
        T_mean = sum(lens) / len(lens)
        val = nq_dec * reps / float(dt.item())
        decode = {"metric": "questions/sec reweighted-decode", "value": val, "unit": "questions/s",
                  "questions": nq_dec, "each_question_once": True, "per_gpu": val / world,
                  "scaling": "strong" if args.config != 5 else "weak",
                  "batch_per_gpu": B, "batches_on_rank0": [len(b) for b in my_batches],
                  "new_tokens": args.decode_tokens, "heads": heads_desc,
                  "scores": ("GPT truthful, -min, /max, stable sort" if args.scores == "gpt" and dsname == "nq"
                             else "ideal: fake 0.1, others 1.0"), "mean_prompt_tokens": round(T_mean, 1),
                  "seconds": float(dt.item()), "repeats": reps,
                  "host_encode_ms_per_question": round(host_ms / len(encs), 3),
                  "note": (f"{nq_dec} {dsname} questions, each decoded once across {world} rank(s) "
                           "(cram_amd.dist.decode_sharded: LPT on prompt length, batches of <= batch_per_gpu rows, "
                           "answers all-gathered); packed varlen prefill + graph-replayed greedy steps, EOS ignored "
                           "(random weights)")}
        if phases:
            decode["leg_roofline"] = decode_leg_roofline(spec, phases, mdtype)
        if my_batches and args.full:
            b0 = my_batches[0]
            decode["attention_roofline"] = decode_attention_roofline(eng, [dev_prompts[i] for i in b0],
                                                                     [ws[i] for i in b0], heads, args.decode_tokens,
                                                                     dev)
        # the CPU baseline's questions: the ones nearest the mean prompt length
        qcs = sorted(range(nq_dec), key=lambda i: (abs(lens[i] - T_mean), i))[:max(1, args.cpu_decode_questions)]
        dec_cpu_input = ([(qc, prompts[qc], ws[qc]) for qc in qcs], heads)
        log(f"[rank {rank}] decode: {decode['value']:.2f} questions/s ({nq_dec} questions, T mean {T_mean:.0f}); "
            f"decode attention {decode.get('attention_roofline', {}).get('achieved', 0):.0f} GB/s")
        del dev_prompts

    # ------------------------------------------------------------------ CPU baselines (rank 0, any N)
    # the reference's own algorithm on the host cores (oracle/cpu_baseline.py): IE units (config 3) and the hooked
    # greedy decode of one question (configs 2-5), sampled and extrapolated, after the timed regions.  At N > 1 the
    # north star wants the CPU hook path next to the GPU numbers in the same run: rank 0 times it after every rank
    # has left its timed regions; the other ranks wait at the final barrier (process-group timeout: cdist.init)
    cpu = cpu_dec = None
    want_ie = ie is not None
    want_dec = decode is not None and args.cpu_decode_steps > 0
    if rank == 0 and not args.no_cpu_baseline and (want_ie or want_dec):
        from oracle import cpu_baseline
        t0 = time.time()
        cpu_model = cpu_baseline.hf_model_from_engine(eng)
        log(f"[rank 0] CPU copy of the model in {time.time() - t0:.0f}s")
        if want_ie:
            qi, ids, w, ans = ie["work"][0]
            units_s = cpu_baseline.sample_units(L, H, max(1, args.cpu_units))
            r = cpu_baseline.time_ie_units(cpu_model, ids.cpu(), w, ans.cpu(), units_s, log=log)
            sp_ = r["spread"]
            lay_s = sorted(set(l for l, _ in units_s))
            cpu = {"value": r["units_per_s"], "unit": "heads/s", "cores": r["cores"], "kind": "port",
                   "sample": f"{r['units']} IE units = 1 question x {len(lay_s)} layers {lay_s} x "
                             f"{len(set(h for _, h in units_s))} heads (hooked full forward + full-vocab logits + "
                             f".item(), re_weighting.py:162-171) of NQ question {qi} at T'={ids.numel()}, after 1 "
                             f"un-hooked forward; {r['seconds']:.1f}s; {result['dtype']} torch CPU; extrapolates "
                             f"linearly per unit",
                   "unit_seconds": {"min": round(sp_["min_s"], 3), "median": round(sp_["median_s"], 3),
                                    "max": round(sp_["max_s"], 3)}}
            log(f"[rank 0] cpu baseline {cpu['value']:.4f} heads/s on {cpu['cores']} cores")
        if want_dec:
            qlist, hd = dec_cpu_input
            runs = []
            for qc, ids, w in qlist:
                # long prompts (config 5, ~8k tokens): the hooked forward builds a dense [H, T, T] mask per hooked
                # layer, minutes per question on the host, so the sample runs the first 2 layers and scales per layer
                k_layers = args.cpu_decode_layers if args.cpu_decode_layers >= 0 else (2 if ids.numel() > 4096 else 0)
                r = cpu_baseline.time_decode(cpu_model, ids.cpu(), w, hd if hd else
                                             {l: list(range(H)) for l in range(L)},
                                             new_tokens=args.decode_tokens, sampled_steps=args.cpu_decode_steps,
                                             layers=k_layers, log=log)
                runs.append((qc, r))
            tot_s = sum(r["question_s"] for _, r in runs)
            r = runs[0][1]
            cpu_dec = {"value": len(runs) / tot_s, "unit": "questions/s", "cores": r["cores"], "kind": "port",
                       "method": "sampled + extrapolated",
                       "sample": (f"{len(runs)} question(s) ({dsname} #{', #'.join(str(q) for q, _ in runs)}: "
                                  f"{', '.join(str(x['prompt_tokens']) for _, x in runs)} prompt tokens, {r['heads']} "
                                  f"hooked heads"
                                  + (f" in the first {r['layers_run']} of {r['layers']} layers, times scaled by "
                                     f"{r['layers']}/{r['layers_run']}" if r["layers_run"] < r["layers"] else "")
                                  + "): hooks on the selected heads + greedy generate "
                                  f"(re_weighting.py:115-138) of 1 + {r['sampled_steps']} tokens each, "
                                  f"{sum(x['seconds'] for _, x in runs):.1f}s; per question prefill + "
                                  f"{args.decode_tokens - 1} x median step = "
                                  f"{', '.join('%.1f' % x['question_s'] for _, x in runs)}s at {args.decode_tokens} new "
                                  f"tokens; value = questions / summed seconds; {result['dtype']} torch CPU, batch 1 "
                                  f"as the reference"),
                       "prefill_s": [round(x["prefill_s"], 3) for _, x in runs],
                       "step_seconds": [{k: round(v, 4) for k, v in x["step_s"].items()} for _, x in runs]}
            decode["cpu_baseline"] = cpu_dec
            decode["speedup_vs_cpu"] = round(decode["value"] / cpu_dec["value"], 1)
            log(f"[rank 0] cpu decode baseline {cpu_dec['value']:.5f} questions/s on {cpu_dec['cores']} cores")
        del cpu_model
        log(f"[rank 0] CPU baselines took {time.time() - t0:.0f}s")

    if rank == 0:
        if ie is not None:
            kt = ie["kt"]
            roof = None
            if kt is not None and kt["total_ms"] > 0:
                ach = kt["flops"] / (kt["total_ms"] * 1e-3) / 1e12
                kname = ops.prefill_kernel_name(result["dtype"], spec.num_heads, spec.num_kv_heads,
                                                int(ie["work"][0][1].numel()))
                roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": None,
                        "kernel": f"{kname} ({result['dtype']}, d = 128: credibility-biased causal GQA flash "
                                  f"attention, {result['dtype']} MFMA)",
                        "launches": kt["launches"], "avg_launch_ms": round(kt["avg_ms"], 4),
                        "flops_per_launch": kt["flops"] / kt["launches"],
                        "algorithmic_bytes_per_launch": kt["bytes"] / kt["launches"],
                        "hbm_gbs_algorithmic": round(kt["bytes"] / (kt["total_ms"] * 1e-3) / 1e9, 1)}
                if os.path.exists(PMC_FILE):
                    pmc = json.load(open(PMC_FILE))
                    ratio = pmc["traffic_over_algorithmic"]
                    cur = _b.kernel_source_hash()
                    same_kernel = f"{kname}(" in pmc.get("kernel", "") and result["dtype"] == "bf16"
                    if pmc.get("kernel_source_hash") == cur and not same_kernel:
                        roof["traffic_note"] = (f"PMC evidence {pmc['source']} was measured on {pmc.get('kernel')} "
                                                f"(bf16): not this run's {kname} ({result['dtype']}), not applied")
                    elif pmc.get("kernel_source_hash") == cur:
                        roof["traffic"] = round(ratio * roof["algorithmic_bytes_per_launch"])
                        roof["traffic_note"] = (f"HBM bytes/launch = PMC (FETCH_SIZEx2 + WRITE_SIZE, {pmc['source']}, "
                                                f"kernel source {cur}) / algorithmic = {ratio:.4f} at the sweep shape "
                                                f"B=33 T=962, x this run's algorithmic bytes per launch")
                        # rocprofv3's own view of the same kernel (tools/pmc_to_json.py): MFMA utilisation and HBM
                        # rate against the gfx950 peaks, at the sweep shape, from the PMC passes of this build
                        roof["rocprof"] = {k: pmc[k] for k in PMC_KEYS if k in pmc}
                        roof["mfma_busy"] = pmc.get("mfma_busy")
                    else:
                        roof["traffic_note"] = (f"PMC evidence {pmc['source']} was measured on kernel source "
                                                f"{pmc.get('kernel_source_hash')}, this build is {cur}: not applied")
            kg = ie["kg"]
            dom = None
            if kg is not None and kg["total_ms"] > 0:
                gtf = kg["flops"] / (kg["total_ms"] * 1e-3) / 1e12
                dom = {"kernel": (f"every {result['dtype']} projection GEMM of the step: gemm_w4_kernel "
                                  f"({kg['cram_share']:.3f} of the GEMM time), the split-K tail of o_proj / down_proj "
                                  f"and the library calls left (F.linear: the baseline forward's o_proj / down, "
                                  f"lm_head rows)"),
                       "bound": "mfma", "achieved": round(gtf, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                       "frac": round(gtf / PEAK_BF16_TFLOPS, 4), "launches": kg["launches"],
                       "avg_launch_ms": round(kg["avg_ms"], 4), "flops_per_launch": kg["flops"] / kg["launches"],
                       "share_of_step": round(kg["total_ms"] * 1e-3 / ie["elapsed"], 4),
                       "note": "timed live with HIP events on the launch stream"}
            # the dominant kernel of the step (the contract's `roofline`): gemm_w4_kernel over all its epilogues
            kc = ie["kc"]
            roof_attn = roof
            if kc is not None and kc["total_ms"] > 0:
                ach = kc["flops"] / (kc["total_ms"] * 1e-3) / 1e12
                roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": None,
                        "kernel": (f"gemm_w4_kernel ({result['dtype']} MFMA 16x16x32, 256 x 256 tiles; every epilogue: "
                                   "q/k/v + RoPE, o_proj / down_proj + residual, gate/up + SiLU-mul)"),
                        "launches": kc["launches"], "avg_launch_ms": round(kc["avg_ms"], 4),
                        "flops_per_launch": kc["flops"] / kc["launches"],
                        "algorithmic_bytes_per_launch": kc["bytes"] / kc["launches"],
                        "share_of_step": round(kc["total_ms"] * 1e-3 / ie["elapsed"], 4),
                        "note": "timed live with HIP events on the launch stream over the timed region; the attention "
                                "kernel's roofline is 'roofline_attention'"}
                if os.path.exists(GEMM_PMC_FILE):
                    gp = json.load(open(GEMM_PMC_FILE))
                    cur = _b.gemm_source_hash()
                    if gp.get("kernel_source_hash") == cur:
                        ratio = gp["traffic_over_algorithmic"]
                        roof["traffic"] = round(ratio * roof["algorithmic_bytes_per_launch"])
                        roof["traffic_note"] = (f"HBM bytes/launch = PMC (FETCH_SIZEx2 + WRITE_SIZE, {gp['source']}, "
                                                f"GEMM source {cur}) / algorithmic = {ratio:.4f} at the dominant launch "
                                                f"(gate/up + SiLU-mul, M = 29,184), x this run's algorithmic bytes per "
                                                f"launch")
                        roof["rocprof"] = {k: gp[k] for k in PMC_KEYS if k in gp}
                        roof["mfma_busy"] = gp.get("mfma_busy")
                    else:
                        roof["traffic_note"] = (f"GEMM PMC evidence {gp['source']} was measured on GEMM source "
                                                f"{gp.get('kernel_source_hash')}, this build is {cur}: not applied")
            step_tf = ie["flops"] / ie["elapsed"] / 1e12
            result.update({
                "value": round(ie["value"], 3), "unit": "heads/s",
                "ms_per_step": round(ie["elapsed"] * 1e3 / args.steps, 2), "scaling": "weak",
                "data": f"synthetic: random-init {name} weights; rebuilt NQ-1000 prompts via offline BPE tokenizer",
                "config": {"workload": (f"{name} Find_Best_Heads IE sweep, {L} layers x {H} heads per question, "
                                        "scores [0,1,1,1,1], 1 NQ question per GPU per step (config 3; decode = config 2)")
                                       if not args.position_sweep else
                                       (f"{name} casual_tracing_per_head_with_position (find_best_heads.py:61-110): "
                                        f"{L} layers x {H} heads x fake passage at positions 0..4 per question, "
                                        "1 NQ question per GPU per step"),
                           "questions_per_step": world,
                           "units_per_question": L * H * (5 if args.position_sweep else 1),
                           "question_order": "nearest the mean NQ prompt length first; steps x N questions dealt to "
                                             "ranks by cram_amd.dist.plan (LPT on token counts)",
                           "mean_prompt_tokens": round(ie["mean_T"], 1),
                           "parallelism": f"dp{world} question-sharded + RCCL all-gather of IE"},
                "roofline": roof,
                "roofline_attention": roof_attn,
                "dominant_kernel": dom,
                "step_roofline": {"bound": "mfma", "achieved": round(step_tf, 2), "peak": PEAK_BF16_TFLOPS * world,
                                  "unit": "TFLOP/s", "frac": round(step_tf / (PEAK_BF16_TFLOPS * world), 4),
                                  "flops_per_question": ie["flops"] / max(1, world * args.steps),
                                  "flops_definition": "algorithmic, SURVEY §8(d) with the prefix skip: baseline "
                                                      "forward + per layer the biased attention and 32 variants "
                                                      "through the layers above, the last layer's q / attention / "
                                                      "MLP on the answer rows only (sweep.sweep_flops)",
                                  "executed_flops_per_question": ie["flops_executed"] / max(1, world * args.steps),
                                  "executed_note": ("+ the un-perturbed 33rd variant per batch, " if ie["base_variant"]
                                                    else "") + "+ the GEMMs' pad rows, the baseline's last-layer q "
                                                               "over every row (sweep.sweep_flops_executed); not "
                                                               "credited to frac"},
                "cpu_baseline": cpu, "decode": decode})
            if cpu:
                result["speedup_vs_cpu"] = round(ie["value"] / cpu["value"], 1)
        else:
            wl = {2: f"{name} {dsname.upper()}-1000 reweighted decode ({heads_desc}, ideal scores)",
                  4: f"{name} TriviaQA-1000 reweighted decode ({heads_desc}, ideal scores)",
                  5: f"{name} NQ 20 retrieved docs (~8k tokens) reweighted decode ({heads_desc})"}[args.config]
            result.update({"metric": METRIC + f" [config {args.config}: decode]", "value": round(decode["value"], 3),
                           "unit": "questions/s", "ms_per_step": round(decode["seconds"] * 1e3 / decode["repeats"], 2),
                           "scaling": decode["scaling"],
                           "data": f"synthetic: random-init {model} weights; rebuilt {dsname} prompts",
                           "config": {"workload": wl, "questions": decode["questions"],
                                      "batch_per_gpu": decode["batch_per_gpu"],
                                      "new_tokens": decode["new_tokens"], "mean_prompt_tokens": decode["mean_prompt_tokens"],
                                      "parallelism": f"dp{world} replicas, each question decoded once "
                                                     f"(cram_amd.dist.decode_sharded)"},
                           "roofline": decode.get("attention_roofline"), "cpu_baseline": cpu_dec, "decode": decode})
            if cpu_dec:
                result["speedup_vs_cpu"] = decode["speedup_vs_cpu"]
        if args.dump_outputs:
            import numpy as np
            arrays = {}
            if ie is not None:
                arrays["ie"] = ie["last_step"].float().cpu().numpy()
            if answers is not None:                 # token ids (< 2^24: exact in float32), the last repeat's
                arrays["decode_answers"] = np.asarray(answers, dtype=np.float32)
            dump_outputs(args.dump_outputs, arrays)
        print(json.dumps(result), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def run_config1(args):
    """BASELINE config 1: GPT-2-small (12 x 12 heads, d 64, random init), the first 8 NQ questions x 5 passages,
    ideal scores [0.1, 1, 1, 1, 1], all heads re-weighted (layers_to_be_modified = {}), greedy decode of a fixed
    32 tokens at batch 1 exactly as run_RAG_with_attention_weighting runs it (transformers generate), with the
    cram_hip kernels on 1 GPU; next to it the same decode through the dense-mask hook on the host cores."""
    import torch
    from transformers import AutoTokenizer, GPT2Config, GPT2LMHeadModel
    from cram_amd import attention as A
    from cram_amd import spans
    from cram_amd.bias import CredibilityBias, all_heads
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cfg = GPT2Config(n_layer=12, n_head=12, n_embd=768, n_positions=1024, vocab_size=50257)
    A.register()
    cpu_model = GPT2LMHeadModel(cfg).to(torch.bfloat16).eval()
    import copy
    gpu_model = GPT2LMHeadModel(copy.deepcopy(cfg)).to(torch.bfloat16).eval()     # own config: own attention impl
    gpu_model.load_state_dict(cpu_model.state_dict())
    gpu_model.set_attn_implementation(A.IMPL_NAME)
    gpu_model = gpu_model.to(dev)
    tok = AutoTokenizer.from_pretrained(os.path.join(REPO, "data", "tok_llama3"))
    name = "gpt2-small"                                  # no chat branch: raw template (re_weighting.py:96-97)
    data = load_dataset("nq")[:8]
    L, H = cfg.n_layer, cfg.n_head
    heads = all_heads(L, H)
    prompts = []
    for rec in data:
        _, enc, w, _ = spans.encode(tok, name, rec["question"], rec["ori_fake"] + rec["reranked_dense_ctxs"],
                                    [0.1, 1, 1, 1, 1], "")
        prompts.append((enc["input_ids"], w))
    gen = dict(do_sample=False, max_new_tokens=32, min_new_tokens=32, pad_token_id=0)

    def run_gpu():
        outs = []
        for ids, w in prompts:
            cb = CredibilityBias.build([w], heads, L, H, dev)
            idd = ids.to(dev)
            with A.reweighting(gpu_model, cb), torch.no_grad():
                outs.append(gpu_model.generate(input_ids=idd, attention_mask=torch.ones_like(idd), **gen))
        return outs

    run_gpu()                                             # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(max(1, args.steps)):
        outs = run_gpu()
    torch.cuda.synchronize()
    gpu_s = (time.perf_counter() - t0) / max(1, args.steps)
    if args.dump_outputs:
        import numpy as np
        new = [o[0, ids.shape[1]:].tolist() for o, (ids, _) in zip(outs, prompts)]     # the 32 generated ids per question
        dump_outputs(args.dump_outputs, {"decode_answers": np.asarray(new, dtype=np.float32)})
    value = len(prompts) / gpu_s
    log(f"[config 1] GPU drop-in: {value:.2f} questions/s ({gpu_s:.2f} s for 8 questions)")
    cpu = None
    if not args.no_cpu_baseline:
        from oracle import cpu_baseline, hook_ref
        torch.set_num_threads(cpu_baseline.cores())
        n_cpu = 2                                         # bounded sample: 2 of the 8 questions
        t0 = time.perf_counter()
        for ids, w in prompts[:n_cpu]:
            hs = hook_ref.register_hooks(cpu_model, heads, hook_ref.log_weight(w))
            try:
                with torch.no_grad():
                    cpu_model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), **gen)
            finally:
                for h in hs:
                    h.remove()
        cs = time.perf_counter() - t0
        cpu = {"value": n_cpu / cs, "unit": "questions/s", "cores": cpu_baseline.cores(), "kind": "port",
               "sample": f"{n_cpu} of the 8 questions, 32 greedy tokens each through transformers + the restated "
                         f"dense-mask hook on every layer (GPT-2 adapter), bf16 CPU, {cs:.1f}s"}
        log(f"[config 1] CPU hook path: {cpu['value']:.3f} questions/s on {cpu['cores']} cores")
    T_mean = sum(ids.shape[1] for ids, _ in prompts) / len(prompts)
    # HBM roofline of the batch-1 decode (what bounds a greedy step of transformers' generate): per generated token
    # every weight once (GPT-2-small: 124M parameters, the tied wte doubling as lm_head) + the visible K and V of every
    # layer; the prefill's reads are counted as one step.  The step is host-launch bound at batch 1 (~100 kernels of
    # microseconds each), so the fraction is small; it is the number to hold against the reference's own batch-1 path.
    n_par = sum(p.numel() for p in gpu_model.parameters())
    kv_key = 2 * cfg.n_layer * cfg.n_embd * 2
    new_t = gen["max_new_tokens"]
    tot_bytes = sum(new_t * n_par * 2 + kv_key * sum(ids.shape[1] + t for t in range(new_t)) for ids, _ in prompts)
    roof = {"bound": "hbm", "achieved": round(tot_bytes / gpu_s / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(tot_bytes / gpu_s / 1e9 / PEAK_HBM_GBS, 5), "traffic": None,
            "kernel": "whole batch-1 greedy decode (transformers generate with the cram_hip attention: prefill_kernel "
                      "/ decode_kernel d = 64, library GEMMs)",
            "bytes_per_question": tot_bytes / len(prompts),
            "note": "algorithmic bytes = weights once per generated token + visible K/V; batch 1 as the reference "
                    "(re_weighting.py:40), launch-bound"}
    print(json.dumps({
        "metric": METRIC + " [config 1: GPT-2-small reweighted decode]", "value": round(value, 3),
        "unit": "questions/s", "n_gpus": 1, "steps": args.steps, "warmup": 1, "ms_per_step": round(gpu_s * 1e3, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic: random-init GPT-2-small weights; first 8 rebuilt NQ prompts (raw template)",
        "config": {"workload": "GPT-2-small, 8 NQ questions x 5 retrieved docs, batch-1 hooked-decode shape, all "
                               "heads re-weighted, 32 new tokens",
                   "mean_prompt_tokens": round(T_mean, 1), "parallelism": "single GPU, batch 1"},
        "roofline": roof, "cpu_baseline": cpu,
        "speedup_vs_cpu": round(value / cpu["value"], 1) if cpu else None}), flush=True)


if __name__ == "__main__":
    main()
