"""The one whole-model harness of the suite: a weight family's committed reference fixtures (tests/golden/<prefix><cfg>.bgld, recorded from the GENUINE reference's
llama_decode by that family's generator via oracle/harness/ref_run.cpp), the deterministic synthetic GGUF regenerated for each (size, sha256 of the first 64 MiB
and xxh3-128 of the whole file checked against the fixture), and the runners that hold an implementation to every greedy token, 32 probe logits per step, the top
logit and a 64-bit digest of ALL logits of every step — bit for bit.  A plain helper module (as goldenio.py); every function takes its family explicitly."""
import importlib.util
import os

import numpy as np

from goldenio import load_bgld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Family:
    """a weight family: its name, the prefix of its fixture files and its generator module (tests/golden/gen_<name>_fixtures.py)"""

    def __init__(self, name, prefix):
        self.name, self.prefix, self.gen = name, prefix, _load("gen_%s_fixtures" % name)

    def shape(self, cfg):
        """(model kwargs, n_prompt, n_decode, n_ctx) of a CONFIGS entry: the generators write (kwargs, n_prompt, n_decode, n_ctx), (kwargs, recipe, ...) and
        (kwargs, recipe kwargs, tied, ...) — the model first, the three counts last"""
        c = self.gen.CONFIGS[cfg]
        return (c[0],) + tuple(c[-3:])

    def fixture_path(self, cfg):
        return os.path.join(GOLDEN, "%s%s.bgld" % (self.prefix, cfg))

    def ensure_model(self, cfg, directory):
        """the family's synthetic GGUF of cfg in `directory`, written on first use"""
        if self is not FULLSIZE:
            return self.gen.ensure_model(cfg, directory)
        mp = self.gen.model_path                              # gen_fullsize_fixtures.ensure_model takes no directory: it asks model_path(cfg)
        self.gen.model_path = lambda c: mp(c, directory)
        try:
            return self.gen.ensure_model(cfg)
        finally:
            self.gen.model_path = mp


FULLSIZE, LOWBIT, LEGACY, LEGACY1, FLOAT, IQ4NL = FAMILIES = (Family("fullsize", "fullsize_"), Family("lowbit", "lowbit_"), Family("legacy", "legacy_"),
                                                              Family("legacy1", "legacy1_"), Family("float", "float_"), Family("iq4nl", ""))


def digest(logits):
    u = np.ascontiguousarray(logits, np.float32).view(np.uint32).astype(np.uint64)
    i = np.arange(u.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum((u + np.uint64(0x9E3779B97F4A7C15)) * (np.uint64(2) * i + np.uint64(1)), dtype=np.uint64))


def load_fixture(fam, cfg):
    g = load_bgld(fam.fixture_path(cfg))
    txt = open(fam.fixture_path(cfg) + ".txt").read().split()
    kv = dict(t.split("=", 1) for t in txt if "=" in t)
    return dict(tokens=g["tokens"], digest=g["digest"].copy().view("<u8").reshape(-1), pidx=g["probe_idx"], probes=g["probe_logits"], top=g["top_logit"],
                gguf_bytes=int(kv["gguf_bytes"]), gguf_sha=kv["gguf_sha256_first64MiB"], gguf_xxh=kv["gguf_xxh3_128"])


def model_for(fam, cfg, fx):
    d = "/tmp"
    for cand in ("/dev/shm", "/tmp"):                         # the first writable directory that has the file already or room for it
        if os.path.isdir(cand) and os.access(cand, os.W_OK):
            st = os.statvfs(cand)
            if os.path.exists(fam.gen.model_path(cfg, cand) + ".done") or st.f_bavail * st.f_frsize > fx["gguf_bytes"] + (1 << 30):
                d = cand
                break
    p = fam.ensure_model(cfg, d)
    sha, size = FULLSIZE.gen.file_digest(p)
    assert size == fx["gguf_bytes"] and sha == fx["gguf_sha"], "the regenerated synthetic GGUF differs from the one the reference evaluated"
    assert FULLSIZE.gen.file_digest_full(p) == fx["gguf_xxh"], "the regenerated synthetic GGUF differs from the one the reference evaluated (whole-file digest)"
    return p


def check_step(fx, k, logits, what):
    assert int(np.argmax(logits)) == int(fx["tokens"][k]), "%s: arg-max token of step %d differs from the reference" % (what, k)
    assert np.array_equal(logits[fx["pidx"]].view(np.uint32), fx["probes"][k].view(np.uint32)), "%s: probe logits of step %d differ" % (what, k)
    assert np.float32(logits.max()).view(np.uint32) == fx["top"][k].view(np.uint32), "%s: top logit of step %d differs" % (what, k)
    assert digest(logits) == int(fx["digest"][k]), "%s: digest of all logits of step %d differs" % (what, k)


def prompt_of(n_prompt, V):
    return [(7919 * i + 13) % V for i in range(n_prompt)]


def run_config(bamd, fam, cfg, stepwise, want_aql=False):
    """the prompt in micro-batches of 512, `stepwise` single-token steps checked one by one, the rest through the device-side greedy loop"""
    fx = load_fixture(fam, cfg)
    assert np.isfinite(fx["probes"]).all() and np.isfinite(fx["top"]).all()
    _, n_prompt, n_decode, n_ctx = fam.shape(cfg)
    path = model_for(fam, cfg, fx)
    m = bamd.Model(path)
    ctx = bamd.Context(m, n_ctx)
    prompt = prompt_of(n_prompt, m.n_vocab)
    for i in range(0, n_prompt, 512):                         # micro-batches of 512, as cpp/bridge.cpp feeds a prompt (n_batch chunks)
        lg = ctx.decode(prompt[i:i + 512], i)
    check_step(fx, 0, lg, cfg + " prompt")
    n_past = n_prompt
    for k in range(1, stepwise + 1):                          # step by step: every step's logits against the fixture
        lg = ctx.decode([int(fx["tokens"][k - 1])], n_past); n_past += 1
        check_step(fx, k, lg, cfg + " decode")
    rest = n_decode - stepwise
    if rest > 0:                                              # the device-side greedy loop for the remaining steps
        out, _ = ctx.generate_greedy(n_past, rest)
        assert list(out[:rest + 1]) == [int(t) for t in fx["tokens"][stepwise:n_decode + 1]], cfg + ": greedy tokens differ from the reference"
        check_step(fx, n_decode, ctx.last_logits(), cfg + " last greedy step")
        if want_aql:
            assert ctx.aql_runs() > 0, cfg + ": the greedy loop did not run on the own AQL queue"
    ctx.close(); m.close()


def run_config_through_stages(bamd, fam, cfg, ranges, n_steps):
    """the same fixture through a CHAIN of layer-split stages on this GPU (one Model slice + Context per stage, hidden state handed over as a device buffer on a
    side stream, every stage replaying its own captured stage graph): the prompt as ONE micro-batch through bamd_stage_prefill, then n_steps single-token steps
    through bamd_stage_step — every step's logits against the genuine reference's"""
    import torch
    fx = load_fixture(fam, cfg)
    _, n_prompt, n_decode, n_ctx = fam.shape(cfg)
    assert n_prompt <= 512 and n_steps <= n_decode
    path = model_for(fam, cfg, fx)
    n = len(ranges)
    models = [bamd.Model(path, 0, a, b, i == 0, i == n - 1) for i, (a, b) in enumerate(ranges)]
    ctxs = [bamd.Context(m, n_ctx) for m in models]
    E, V = models[0].n_embd, models[-1].n_vocab
    prompt = prompt_of(n_prompt, V)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        stream = torch.cuda.current_stream().cuda_stream
        hid = [torch.zeros(n_prompt * E, dtype=torch.float32, device="cuda") for _ in range(2)]
        for i, c in enumerate(ctxs):
            hin = None if i == 0 else hid[(i - 1) & 1].data_ptr()
            hout = None if i == n - 1 else hid[i & 1].data_ptr()
            if not c.stage_prefill(prompt if i == 0 else None, n_prompt, 0, hin, hout, i == n - 1, stream):
                # a stage without batched kernels for its shape (the 70B widths without side tables: BAMD_PREFILL_AUX=0, no memory for them) declines the micro-batch:
                # the caller's documented fallback (pipeline.HipStage.prefill) is token by token with the same T > 1 semantics — same bits
                for j in range(n_prompt):
                    c.stage_step(prompt[j] if i == 0 else 0, j, None if hin is None else hin + j * E * 4, None if hout is None else hout + j * E * 4,
                                 i == n - 1 and j == n_prompt - 1, True, stream)
        check_step(fx, 0, ctxs[-1].stage_logits(stream), cfg + " prompt through %d stages" % n)
        n_past = n_prompt
        for k in range(1, n_steps + 1):
            t = int(fx["tokens"][k - 1])
            for i, c in enumerate(ctxs):
                hin = None if i == 0 else hid[(i - 1) & 1].data_ptr()
                hout = None if i == n - 1 else hid[i & 1].data_ptr()
                c.stage_step(t, n_past, hin, hout, i == n - 1, False, stream)
            n_past += 1
            check_step(fx, k, ctxs[-1].stage_logits(stream), cfg + " decode through %d stages" % n)
    for c in ctxs:
        c.close()
    for m in models:
        m.close()


def nine_symbol_bridge(bamd, tmp_path, recipe, model_kwargs, type_fn_of, **writer_kwargs):
    """a tiny shape under a recipe, with a tokenizer, through the nine cgo symbols in the call sequence of tests/test_gpu_bridge.py (initContext -> init ->
    doInference on one thread while status / getPromptTokenCount are polled, then the counters): token-identical to generate_greedy on the same file.  Janus is
    set to what makes it the arg-max: scale 1.0 (every repeat factor is 1) and hi = lo = 1.0 (the shortlist is the top candidate alone).  type_fn_of(kwargs) gives
    (type_fn, embd_type) of the model kwargs with the tokenizer's vocabulary size; writer_kwargs go to write_synthetic_llama as they are."""
    import ctypes as C
    import threading
    import time
    from booster_amd import gguf
    from test_gpu_bridge import bind
    lib = bind(bamd)
    vocab = gguf.synthetic_spm_vocab()
    kw = dict(model_kwargs); kw["V"] = len(vocab["tokens"])
    fn, embd = type_fn_of(kw)
    path = str(tmp_path / ("bridge_%s.gguf" % recipe))
    gguf.write_synthetic_llama(path, seed=21, type_fn=fn, embd_type=embd, vocab=vocab, **writer_kwargs, **kw)
    n_predict = 16                                           # (status() is a C string: the continuations of these files hold no NUL byte piece this far, asserted below)
    ctx = lib.initContext(7, path.encode(), 4, 512, 100, 0, 0, 0, 128, n_predict, 0, 0.0, 0.0, 0.8, 40, 0.9, 1.0, 1.1, 64, 1, 200, 1.0, 1.0, 1.0, 42, b"")
    assert ctx, "initContext failed"
    lib.init(b"", b"")
    prompt = b"the cat sat on the hat"
    ids = np.zeros(256, np.int32)
    n_prompt = lib.bamd_bridge_tokenize(ctx, prompt, 0, 1, ids.ctypes.data_as(C.c_void_p), 256)
    assert n_prompt > 0
    job = ("job-" + recipe).encode()
    seen, done = [], threading.Event()

    def poll():
        while not done.is_set():
            seen.append(lib.status(job))
            lib.getPromptTokenCount(job)
            time.sleep(0.001)
    t = threading.Thread(target=poll); t.start()
    n = lib.doInference(7, ctx, job, b"sess", prompt)
    done.set(); t.join()
    text = lib.status(job)
    assert lib.getPromptTokenCount(job) == n_prompt and n_prompt + 1 <= n <= n_prompt + n_predict
    assert all(text.startswith(s) for s in seen if s)
    # the same file through the level-1 API: prompt, then the device greedy loop
    lib.bamd_bridge_token_to_piece.restype = C.c_void_p
    lib.bamd_bridge_token_to_piece.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

    def piece(i):
        ln = C.c_int(0)
        ptr = lib.bamd_bridge_token_to_piece(ctx, int(i), C.byref(ln))
        return C.string_at(ptr, ln.value)
    m = bamd.Model(path)
    c = bamd.Context(m, 128)
    first = int(np.argmax(c.decode([int(v) for v in ids[:n_prompt]], 0)))
    out, _ = c.generate_greedy(n_prompt, n_predict - 1)       # out[0] = the arg-max of the prompt's logits, then one token per step
    c.close(); m.close()
    toks = [int(v) for v in out[:n_predict]]
    assert toks[0] == first
    eos = vocab["eos_token_id"]
    if eos in toks:                                          # the bridge stops behind an end-of-generation token
        toks = toks[:toks.index(eos) + 1]
    want = b"".join(piece(i) for i in ids[:n_prompt]) + b"".join(piece(i) for i in toks)
    assert b"\0" not in want, "a generated piece is the NUL byte: status() cannot carry it, shorten n_predict"
    assert text == want, "bridge text differs from the greedy tokens' pieces:\n%r\n%r" % (text, want)
    assert n == n_prompt + len(toks) - 1                     # the prompt batch, then one evaluation per generated token except the last
