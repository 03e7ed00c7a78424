"""Flagship serving benchmark: OpenAI /v1/chat/completions with 4k-token
bodies through the gateway to a mock upstream (BASELINE.json config #1 +
the GPU token-accounting path of config #2 when a GPU is present).

Topology: one rank per GPU (the driver launches N ranks via torchrun).
Within a rank, the shard is a process GROUP: ``--workers`` HTTP worker
processes each run a full gateway + mock upstream + load loop (CPython's
GIL caps a single asyncio process near ~3k req/s; the MI355X node pairs
256 CUs with ~128 EPYC cores, so the shard design uses processes the way
Envoy uses worker threads). Each worker pins its GPU work to the rank's
GPU; kernels from all workers interleave on the device.

Timing contract: W untimed warmup steps per worker, then exactly K steps,
bracketed by a distributed barrier + torch.cuda.synchronize on both
sides; the value is the whole-job aggregate request rate over all ranks
and workers computed from the MAX elapsed time. Rank 0 prints ONE JSON
line. One step = ``--waves`` sequential waves of ``--batch`` concurrent
requests per worker (default 50×32), sized so the driver's standard
``--steps 20 --warmup 5`` run times a multi-second region at steady
state — short timed regions under-report by ~30% because connection
pools, GC state, and the GPU admission pipeline are still cold
(round-1 finding: 20×1-wave steps measured 49.8k on a config that
sustains 72.8k over 9.6M requests).

The harness confines itself to the CPUs of one NUMA node (the GPU's,
when known) before it starts any thread, so the rate does not move with
where the scheduler happens to place the loopback peers; ``--no-pin``
leaves the affinity alone (figures in ``_pin_to_numa_node``).

The ``metric`` string names two things; the request rate is ``value``,
and the latency half (``config.p50_added_latency_ms``) is filled only
with ``--full``. If the native extension cannot be imported a plain run
still falls back to the Python lean front, visible only as
``config.front == "lean"`` — compare builds on ``front == "fast"``;
``--dump-outputs`` refuses that fallback.

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the line. ``--full`` adds the secondary
measurements (the warm direct-to-upstream latency baseline behind
``p50_added_latency_ms``; the state-sync tick timing on multi-rank runs).
``--dump-outputs DIR`` writes what the timed path produced in its last
step as ``DIR/<name>.npy`` (see ``dump_outputs``); the payloads, the
tokenizer tables and the upstream's canned body are fixed, so two builds
can be compared output for output.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import multiprocessing as mp
import os
import statistics
import time

import torch

WORDS = (
    "the quick brown fox jumps over the lazy dog while seventeen engineers "
    "profile matrix kernels on a liquid cooled accelerator node during the "
    "long afternoon of benchmark season"
).split()

# `created` stamp of the mock upstream's canned completion (fixed, so the
# bytes the gateway relays are identical from run to run)
BENCH_CREATED = 1700000000

# server-side accounting counters written by --dump-outputs, in file order
DUMP_COUNTERS = ("requests", "responses_2xx", "gpu_tokens", "input_tokens",
                 "output_tokens", "total_tokens", "bytes_in", "bytes_out",
                 "cache_hits", "cache_misses")


def dump_outputs(out_dir: str, bodies: list, stats0: dict, stats1: dict,
                 steps: int) -> None:
    """Write what the timed path produced as float64 .npy files.

    responses.npy  [connections, max_len]: the response body every client
        connection received for the FINAL request of the last timed step,
        one byte value per element, rows padded with -1.
    response_lengths.npy  [connections]: body length per row.
    accounting_per_step.npy  [len(DUMP_COUNTERS)]: the gateway's counters
        (requests served, GPU-counted prompt tokens, usage tokens charged,
        bytes relayed, semantic-cache hits/misses) accumulated over the
        timed region, per step. Every step issues the same requests, so
        the per-step figure is the region total over --steps.
    A few hundred KB at the default sizes (one short completion body per
    connection), far below any size that would need sampling."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    width = max((len(b) for b in bodies), default=0)
    resp = np.full((len(bodies), width), -1.0, dtype=np.float64)
    for i, b in enumerate(bodies):
        resp[i, : len(b)] = np.frombuffer(b, dtype=np.uint8)
    np.save(os.path.join(out_dir, "responses.npy"), resp)
    np.save(os.path.join(out_dir, "response_lengths.npy"),
            np.array([len(b) for b in bodies], dtype=np.float64))
    acct = np.array([(stats1[k] - stats0[k]) / steps for k in DUMP_COUNTERS],
                    dtype=np.float64)
    np.save(os.path.join(out_dir, "accounting_per_step.npy"), acct)


def _gpu_device(local_rank: int) -> int:
    """Clamp the rank's device (multi-rank rehearsal on fewer GPUs)."""
    import torch as _t

    n = max(_t.cuda.device_count(), 1)
    return local_rank % n


def build_payload(n_tokens: int) -> dict:
    """~n_tokens-token chat body (words ≈ tokens for the synthetic BPE)."""
    words = [WORDS[i % len(WORDS)] for i in range(n_tokens)]
    text = " ".join(words)
    third = len(text) // 3
    return {
        "model": "bench-llm",
        "messages": [
            {"role": "system", "content": "You are a terse assistant. " + text[:third]},
            {"role": "user", "content": text[third : 2 * third]},
            {"role": "assistant", "content": text[2 * third :]},
            {"role": "user", "content": "Summarize in one word."},
        ],
        "max_tokens": 16,
    }


def gateway_config(upstream_port: int) -> dict:
    return {
        "version": "v1",
        "uuid": "bench",
        "llmRequestCosts": [{"metadataKey": "llm_total_token", "type": "TotalToken"}],
        "routes": [
            {
                "name": "bench",
                "headers": [{"name": "x-ai-eg-model", "value": "bench-llm"}],
                "backends": [
                    {
                        "name": "mock-openai",
                        "schema": "OpenAI",
                        "upstream": {"host": "127.0.0.1", "port": upstream_port},
                        "auth": {"apiKey": "sk-bench"},
                    }
                ],
            }
        ],
        "rateLimits": [
            {
                "name": "node-token-budget",
                "metadataKey": "llm_total_token",
                "limit": 10**12,
                "windowS": 3600,
            }
        ],
    }


async def fire_step(client, port, path, payloads, batch, latencies, counter=None,
                    waves: int = 1):
    """One step: ``batch`` closed-loop client slots, each issuing ``waves``
    sequential POSTs via the lean pooled client (batch×waves requests per
    step, one join at the END of the step). Slots are independent — there
    is no per-wave barrier, because a barrier makes every wave wait for
    its straggler and the measured rate collapses to the p99 tail
    (measured on the native front: 28k req/s with per-wave barriers vs
    the server's actual capacity; arrivals also synchronize into bursts).
    ``payloads`` is one bytes object or a pool cycled via ``counter``
    (the semantic-cache mode reuses a payload pool to produce hits)."""

    pool = payloads if isinstance(payloads, list) else [payloads]

    async def slot(i):
        for w in range(waves):
            body = pool[(counter[0] + i + w * batch) % len(pool)] if counter else pool[0]
            t0 = time.perf_counter()
            r = await client.post(
                host="127.0.0.1", port=port, tls=False, path=path,
                headers={"content-type": "application/json"},
                body=body, timeout_s=120.0,
            )
            await r.read()
            r.release()
            assert r.status == 200, f"status {r.status}"
            latencies.append((time.perf_counter() - t0) * 1000.0)

    await asyncio.gather(*(slot(i) for i in range(batch)))
    if counter:
        counter[0] += batch * waves


async def worker_main(args, local_rank: int, ready, go, out_q):

    from aigw.extproc.server import GatewayServer
    from aigw.filterapi import RuntimeConfig, load_config
    from aigw.testing.fastmock import canned_chat_response, start_fast_mock

    use_gpu = torch.cuda.is_available() and not getattr(args, "no_gpu", False)
    if use_gpu:
        torch.cuda.set_device(_gpu_device(local_rank))

    up_server, up_port = await start_fast_mock(
        response=canned_chat_response(prompt_tokens=args.tokens)
    )
    cfg = load_config(gateway_config(up_port))

    cache_mode = getattr(args, "cache_payloads", 0) > 0
    gpu_services = None
    if use_gpu and getattr(args, "gpu_socket", None):
        # one GPU context per SHARD: workers RPC to the rank-primary's
        # admission service (scales past the ~16-worker direct-context
        # knee; see --gpu-service help)
        from aigw.gpu.service import RemoteGPUClient

        gpu_services = RemoteGPUClient(args.gpu_socket, window_ms=args.gpu_window, max_batch=256)
    elif use_gpu:
        from aigw.gpu import GPUServices

        gpu_services = GPUServices(
            device=f"cuda:{local_rank}", n_merges=32768, enable_cache=cache_mode,
            cache_threshold=0.98, window_ms=getattr(args, "gpu_window", 0.1),
            cache_index_dtype="fp8" if getattr(args, "cache_fp8", False) else "bf16",
            max_batch=256,
        )

    server = GatewayServer(RuntimeConfig(cfg), gpu_services=gpu_services)
    from aigw.extproc.lean_front import serve_lean

    _, gw_port, gw_cleanup = await serve_lean(
        server, "127.0.0.1", 0, with_fallback=False
    )

    from aigw.extproc.upstream_client import LeanClient

    if cache_mode:
        # distinct payload pool -> steady-state hit ratio 1 - D/total
        payloads = []
        for i in range(args.cache_payloads):
            pl = build_payload(args.tokens)
            pl["messages"][1]["content"] = f"variant {i}: " + pl["messages"][1]["content"]
            payloads.append(json.dumps(pl).encode())
    else:
        payloads = [json.dumps(build_payload(args.tokens)).encode()]
    client = LeanClient()
    path = "/v1/chat/completions"
    counter = [0]

    # warm the gateway path; --full also warms the direct path and records
    # the warm direct-to-upstream baseline.
    # Warmup is wave-scaled like the timed steps: the lean client's pools,
    # GC steady state and the GPU admission pipeline need hundreds of
    # waves before the shard reaches its sustained rate.
    waves = max(args.waves, 1)
    scratch: list[float] = []
    if args.full:
        for _ in range(max(args.warmup, 1)):
            await fire_step(client, up_port, path, payloads, args.batch,
                            scratch, waves=min(waves, 10))
    for _ in range(args.warmup):
        await fire_step(client, gw_port, path, payloads, args.batch, scratch,
                        counter, waves=waves)
    direct_lat: list[float] = []
    if args.full:
        await fire_step(client, up_port, path, payloads, args.batch,
                        direct_lat, waves=5)
    if use_gpu:
        torch.cuda.synchronize()

    ready.set()
    while not go.is_set():
        await asyncio.sleep(0.001)

    lat: list[float] = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        await fire_step(client, gw_port, path, payloads, args.batch, lat,
                        counter, waves=waves)
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    out_q.put(
        {
            "elapsed": elapsed,
            "requests": args.steps * waves * args.batch,
            "p50": statistics.median(lat),
            "p99": sorted(lat)[max(int(len(lat) * 0.99) - 1, 0)],
            "p50_direct": statistics.median(direct_lat) if direct_lat else None,
        }
    )
    await client.close()
    await gw_cleanup()
    up_server.close()
    await up_server.wait_closed()
    if gpu_services is not None:
        gpu_services.close()


def worker_entry(args, local_rank, ready, go, out_q):
    from aigw.utils import tune_gc

    tune_gc()
    asyncio.run(worker_main(args, local_rank, ready, go, out_q))


# ---- fast-front mode: ONE native C++ gateway per rank ------------------------
#
# The Python-front mode above needs 12 worker processes per shard because
# CPython caps one process near ~6k req/s; the C++ front (csrc/fastpath.cpp)
# serves the whole shard from native threads, so the process group becomes:
# rank primary = gateway (+ GPU admission host), M mock-upstream processes,
# L load-generator processes.


def upstream_entry(args, port_q):
    from aigw.testing.fastmock import canned_chat_response, start_fast_mock

    async def amain():
        srv, port = await start_fast_mock(
            response=canned_chat_response(prompt_tokens=args.tokens)
        )
        port_q.put(port)
        await asyncio.Event().wait()

    asyncio.run(amain())


def loadgen_entry(args, gw_port, direct_port, ready, go, out_q):
    from aigw.utils import tune_gc

    tune_gc()

    async def amain():
        from aigw.extproc.upstream_client import LeanClient

        client = LeanClient()
        payloads = [json.dumps(build_payload(args.tokens)).encode()]
        path = "/v1/chat/completions"
        waves = max(args.waves, 1)
        scratch: list[float] = []
        if args.full:
            for _ in range(max(args.warmup, 1)):
                await fire_step(client, direct_port, path, payloads,
                                args.batch, scratch, waves=min(waves, 10))
        for _ in range(args.warmup):
            await fire_step(client, gw_port, path, payloads, args.batch,
                            scratch, waves=waves)
        direct_lat: list[float] = []
        if args.full:
            await fire_step(client, direct_port, path, payloads, args.batch,
                            direct_lat, waves=5)

        ready.set()
        while not go.is_set():
            await asyncio.sleep(0.001)

        lat: list[float] = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            await fire_step(client, gw_port, path, payloads, args.batch, lat,
                            waves=waves)
        elapsed = time.perf_counter() - t0
        out_q.put(
            {
                "elapsed": elapsed,
                "requests": args.steps * waves * args.batch,
                "p50": statistics.median(lat),
                "p99": sorted(lat)[max(int(len(lat) * 0.99) - 1, 0)],
                "p50_direct": statistics.median(direct_lat) if direct_lat else None,
            }
        )
        await client.close()

    asyncio.run(amain())


def _start_fast_front(args, upstream_ports, gpu_socket, gpu_direct=False,
                      gpu_cache=False):
    """Run the C++ gateway (and its Python fallback app) on a dedicated
    thread/loop in the rank primary; returns (front, port)."""
    import threading

    from aigw.extproc.fast_front import FastFront
    from aigw.extproc.server import GatewayServer
    from aigw.filterapi import RuntimeConfig, load_config

    cfg_dict = gateway_config(upstream_ports[0])
    backends = [
        {
            "name": f"mock-openai-{i}",
            "schema": "OpenAI",
            "upstream": {"host": "127.0.0.1", "port": p},
            "auth": {"apiKey": "sk-bench"},
            "weight": 1,
        }
        for i, p in enumerate(upstream_ports)
    ]
    cfg_dict["routes"][0]["backends"] = backends
    cfg = load_config(cfg_dict)
    server = GatewayServer(RuntimeConfig(cfg))
    front = FastFront(
        server, server.runtime, gpu_socket=gpu_socket or "",
        gpu_window_us=int(args.gpu_window * 1000.0), gpu_max_batch=1024,
        gpu_direct=gpu_direct, gpu_cache=gpu_cache,
        cache_index_dtype="fp8" if getattr(args, "cache_fp8", False) else "bf16",
        gpu_device=_gpu_device(int(os.environ.get("LOCAL_RANK", 0))),
    )
    done = threading.Event()
    state = {}

    def run():
        async def amain():
            state["port"] = await front.start("127.0.0.1", 0)
            done.set()
            await asyncio.Event().wait()

        asyncio.run(amain())

    t = threading.Thread(target=run, daemon=True, name="aigw-fast-front")
    t.start()
    if not done.wait(timeout=600):
        raise RuntimeError("fast front failed to start")
    return front, state["port"]


def gpu_host_entry(socket_path, local_rank, window_ms, ready_evt):
    """One GPU admission-host PROCESS (own GPU context + own GIL): the
    native front shards count batches across several of these — one host
    caps near ~900 MB/s of msgpack-decoded request text (measured:
    36k req/s vs 82k without GPU), so admission decode must scale in
    processes just like the round-1 HTTP workers did."""
    torch.cuda.set_device(_gpu_device(local_rank))
    from aigw.gpu import GPUServices
    from aigw.gpu.service import GPUServiceHost

    async def amain():
        gpu = GPUServices(device=f"cuda:{local_rank}", n_merges=32768,
                          enable_cache=False, window_ms=window_ms, max_batch=1024)
        host = GPUServiceHost(gpu, socket_path)
        await host.start()
        ready_evt.set()
        await asyncio.Event().wait()

    asyncio.run(amain())


def run_fast_mode(args, rank, world, local_rank, use_gpu):
    ctx = mp.get_context("spawn")
    cores = os.cpu_count() or 8
    # the C++ gateway saturates well past what one loadgen generates:
    # size the harness (not the gateway) to the machine — the MI355X node
    # pairs 256 CUs with 128+ EPYC cores; CI containers are much smaller
    n_up = args.upstreams if args.upstreams > 0 else max(1, min(20, cores // 10))
    loadgens = args.workers if args.workers > 0 else max(2, min(24, cores // 5))

    port_q = ctx.Queue()
    up_procs = [ctx.Process(target=upstream_entry, args=(args, port_q))
                for _ in range(n_up)]
    for p in up_procs:
        p.start()
    ports = [port_q.get(timeout=600) for _ in range(n_up)]

    gpu_sockets = []
    gpu_host_procs = []
    gpu_direct = False
    if use_gpu and args.gpu_hosts <= 0:
        # default: in-process HIP admission — the native server launches
        # the BPE kernels itself (no IPC, no extra GPU contexts; the UDS
        # host topology measured 36k single-host / 10k 4-host vs 82k
        # without GPU work)
        gpu_direct = True
        torch.cuda.set_device(_gpu_device(local_rank))
    elif use_gpu:
        n_hosts = args.gpu_hosts
        host_ready = []
        for h in range(n_hosts):
            sock = f"/tmp/aigw-gpu-{rank}-{os.getpid()}-{h}.sock"
            ev = ctx.Event()
            p = ctx.Process(target=gpu_host_entry,
                            args=(sock, local_rank, args.gpu_window, ev))
            p.start()
            gpu_sockets.append(sock)
            gpu_host_procs.append(p)
            host_ready.append(ev)
        for ev in host_ready:
            if not ev.wait(timeout=600):
                raise RuntimeError("GPU admission host failed to start")
    front, gw_port = _start_fast_front(args, ports, gpu_sockets, gpu_direct)

    ready_evts = [ctx.Event() for _ in range(loadgens)]
    go = ctx.Event()
    out_q = ctx.Queue()
    procs = [
        ctx.Process(
            target=loadgen_entry,
            args=(args, gw_port, ports[i % n_up], ready_evts[i], go, out_q),
        )
        for i in range(loadgens)
    ]
    for p in procs:
        p.start()
    for ev in ready_evts:
        if not ev.wait(timeout=900):
            for p in procs + up_procs:
                p.terminate()
            raise RuntimeError("load generator failed to become ready")
    return front, go, out_q, procs, up_procs + gpu_host_procs, loadgens


def _start_gpu_host(socket_path: str, local_rank: int, window_ms: float = 0.1):
    """Run the shard's GPU admission service on a dedicated thread/loop in
    the rank-primary process (the only process owning a GPU context)."""
    import threading

    ready_evt = threading.Event()

    def run():
        torch.cuda.set_device(_gpu_device(local_rank))
        from aigw.gpu import GPUServices
        from aigw.gpu.service import GPUServiceHost

        async def amain():
            gpu = GPUServices(device=f"cuda:{local_rank}", n_merges=32768,
                              enable_cache=False, window_ms=window_ms, max_batch=1024)
            host = GPUServiceHost(gpu, socket_path)
            await host.start()
            ready_evt.set()
            await asyncio.Event().wait()

        asyncio.run(amain())

    t = threading.Thread(target=run, daemon=True, name="aigw-gpu-host")
    t.start()
    if not ready_evt.wait(timeout=600):
        raise RuntimeError("GPU admission service failed to start")
    return t




def _cpu_quota() -> int:
    """Effective CPU budget: the cgroup quota, NOT nproc — gpurun boxes
    expose 256 cores but cap the container at 16 CPUs (cpu.max), and
    oversubscribing the quota earns 100 ms CFS throttle stalls that
    poison p99 (measured: 64 connections -> 78k req/s @ p99 1 ms;
    512 connections -> 19k @ p99 102 ms on the same box)."""
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            parts = open(path).read().split()
            if parts[0] != "max":
                return max(1, int(int(parts[0]) / int(parts[1])))
        except (OSError, ValueError, IndexError):
            pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return max(1, q // p)
    except (OSError, ValueError):
        pass
    return os.cpu_count() or 8


def _parse_cpulist(text: str) -> set:
    cpus = set()
    for part in text.strip().split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def _pin_to_numa_node(device) -> str | None:
    """Confine the harness to the CPUs of ONE NUMA node (the GPU's when
    the PCI topology names it, else the node with most usable CPUs).
    Gateway, mock upstream and load generator talk over loopback; left to
    the scheduler their threads land on both sockets and the rate moves
    with the placement, too much for two runs to be compared. Alternating
    runs at --steps 20 --warmup 5, six each: 125.4-127.1k req/s with the
    pin (p99 1.1-1.4 ms), 111.3-119.8k with --no-pin (p99 1.8-4.8 ms).
    Returns a description for the result line; None when nothing was
    pinned (one node, or a node with fewer CPUs than the quota)."""
    import glob

    allowed = os.sched_getaffinity(0)
    nodes = {}
    for path in glob.glob("/sys/devices/system/node/node[0-9]*/cpulist"):
        cpus = _parse_cpulist(open(path).read()) & allowed
        if cpus:
            nodes[int(path.split("/")[-2][4:])] = cpus
    if len(nodes) < 2:
        return None
    node = None
    if device is not None:
        try:
            p = torch.cuda.get_device_properties(device)
            bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id,
                                        p.pci_device_id)
            node = int(open(f"/sys/bus/pci/devices/{bdf}/numa_node").read())
        except (AttributeError, OSError, ValueError):
            pass
    if node not in nodes:
        node = max(sorted(nodes), key=lambda n: len(nodes[n]))
    if len(nodes[node]) < _cpu_quota():
        return None
    # runtime threads that already exist do not inherit a new mask
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), nodes[node])
        except OSError:  # the thread has exited since the listing
            pass
    return f"numa node {node} ({len(nodes[node])} cpus)"


def _settled_stats(front) -> dict:
    """The front's counters once they have stopped moving: the server
    threads bump them after the client already has its response, so a
    read straight after a load run can miss the last increments (and a
    read straight before the next would then count them there)."""
    stats = front.stats()
    for _ in range(200):
        time.sleep(0.005)
        prev, stats = stats, front.stats()
        if stats == prev and stats["active_connections"] == 0:
            break
    return stats


def run_native_bench(args, rank, world, local_rank, use_gpu, barrier_sync):
    """Single-process native harness: C++ mock upstream + C++ gateway
    (with in-process HIP admission) + C++ closed-loop load generator —
    the Python asyncio harness caps near ~2k req/s per loadgen process
    for 25 KiB bodies and was measured to be the bottleneck, not the
    gateway. Returns (results_row, elapsed_s, workers, front)."""
    import aigw_fast

    from aigw.testing.fastmock import canned_chat_response

    if args.stream:
        from aigw.testing.fastmock import canned_chat_sse

        canned = canned_chat_sse(prompt_tokens=args.tokens,
                                 n_chunks=args.stream_chunks)
    else:
        # fixed `created` stamp: the upstream body is a benchmark INPUT and
        # must be byte-identical from run to run (--dump-outputs)
        canned = canned_chat_response(prompt_tokens=args.tokens,
                                      created=BENCH_CREATED)
    mock = aigw_fast.FastMock()
    up_port = mock.start("127.0.0.1", canned.decode("latin1"))
    gpu_direct = use_gpu
    if gpu_direct:
        torch.cuda.set_device(_gpu_device(local_rank))
    cache_mode = use_gpu and args.cache_payloads > 0
    front, gw_port = _start_fast_front(args, [up_port], None, gpu_direct,
                                       gpu_cache=cache_mode)

    if cache_mode:
        # a fixed pool of distinct payloads: after one cold pass the
        # native cache serves (pool exhausted) hits from the HBM index
        payloads = []
        for i in range(args.cache_payloads):
            pl = build_payload(args.tokens)
            pl["messages"][1]["content"] = f"variant {i}: " + pl["messages"][1]["content"]
            payloads.append(json.dumps(pl).encode())
    else:
        pl = build_payload(args.tokens)
        if args.stream:
            pl["stream"] = True
            pl["stream_options"] = {"include_usage": True}
        payloads = [json.dumps(pl).encode()]
    # the cgroup CPU quota is shared by ALL ranks on a node: divide the
    # measured single-rank sweet spot (quota/4 workers) by the world size
    # so an 8-rank scale run does not earn CFS throttle stalls. Without
    # GPU admission the relay threads never sleep (no ~1ms batch wait
    # parking them), so the CFS knee arrives at half the connection
    # count — size nogpu mode to quota/8 (64 conns at the 16-CPU quota:
    # 82k @ p99 0.9ms, vs 33k @ p99 88ms at 128 conns). Cache mode is the
    # other direction: every request sleeps a full embed+top-k batch
    # cycle, so it takes ~3*quota/4 workers to keep the quota busy
    # (vectorized-meanpool kernels: 104.1k @ w8, 112.0k @ w10,
    # 115.3k @ w12 on the 16-CPU quota).
    if cache_mode:
        workers = args.workers if args.workers > 0 else max(
            1, min(12, (3 * _cpu_quota() // 4) // max(world, 1)))
    else:
        div = 4 if gpu_direct else 8
        workers = args.workers if args.workers > 0 else max(
            1, min(8, _cpu_quota() // (div * max(world, 1))))
    conns = args.batch * workers
    waves = max(args.waves, 1)
    path = "/v1/chat/completions"

    # warmup (gateway); --full also records the warm direct-to-upstream
    # baseline that p50_added_latency_ms is measured against
    aigw_fast.run_load_pool("127.0.0.1", gw_port, path, payloads, conns,
                            max(args.warmup, 1) * waves)
    direct = None
    if args.full:
        direct = aigw_fast.run_load_pool("127.0.0.1", up_port, path, payloads,
                                         conns, 5)
    if use_gpu:
        torch.cuda.synchronize()

    dump = bool(args.dump_outputs) and rank == 0
    stats0 = _settled_stats(front) if dump else None
    barrier_sync()
    t0 = time.perf_counter()
    res = aigw_fast.run_load_pool("127.0.0.1", gw_port, path, payloads, conns,
                                  args.steps * waves, capture_last=dump)
    if use_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    barrier_sync()
    assert res["errors"] == 0, f"load errors: {res}"
    if dump:
        dump_outputs(args.dump_outputs, res["last_bodies"], stats0,
                     _settled_stats(front), args.steps)
    row = {
        "elapsed": elapsed,
        "requests": res["completed"],
        "p50": res["p50_ms"],
        "p99": res["p99_ms"],
        "p50_direct": direct["p50_ms"] if direct else None,
    }
    mock.stop()
    return row, elapsed, workers, front


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="concurrent requests per wave")
    ap.add_argument("--waves", type=int, default=250,
                    help="sequential requests per connection per step; "
                         "sizes the timed region so the driver's "
                         "--steps 20 runs a multi-second region at the "
                         "native harness's ~70-80k req/s")
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--workers", type=int, default=0,
                    help="HTTP worker processes per shard (0 = auto)")
    ap.add_argument("--no-gpu", action="store_true",
                    help="disable GPU token accounting (contention diagnosis)")
    ap.add_argument("--stream", action="store_true",
                    help="streamed serving: clients send stream:true and "
                         "the mock answers an SSE chunk sequence; measures "
                         "the native relay + usage-tap path")
    ap.add_argument("--stream-chunks", type=int, default=16,
                    help="SSE content chunks per streamed response")
    ap.add_argument("--cache-fp8", action="store_true",
                    help="fp8 (e4m3) semantic-cache index instead of bf16")
    ap.add_argument("--cache-payloads", type=int, default=0,
                    help="semantic-cache mode: cycle this many distinct "
                         "payloads per worker (0 = cache off); steady-state "
                         "hit ratio approaches 1")
    ap.add_argument("--front", choices=["lean", "fast"], default="fast",
                    help="fast = native C++ gateway (csrc/fastpath.cpp), one "
                         "per rank; lean = Python lean front across --workers "
                         "processes (the round-1 configuration)")
    ap.add_argument("--upstreams", type=int, default=0,
                    help="fast mode: mock-upstream processes per rank (0 = 8)")
    ap.add_argument("--gpu-hosts", type=int, default=0,
                    help="fast mode: 0 = in-process HIP admission (default); "
                         "N>0 = N UDS admission-host processes per rank")
    ap.add_argument("--harness", choices=["native", "python"], default="native",
                    help="fast mode: native = C++ loadgen/mock in one "
                         "process (default; the Python harness IS the "
                         "bottleneck above ~50k req/s); python = asyncio "
                         "loadgen + mock processes")
    ap.add_argument("--gpu-window", type=float, default=0.1,
                    help="GPU micro-batch window per worker, ms")
    ap.add_argument("--gpu-service", action="store_true",
                    help="route GPU work through ONE per-shard admission "
                         "service over IPC instead of per-worker GPU "
                         "contexts. Wins above ~16 workers/shard (48k req/s "
                         "@40w measured) at higher p50; direct contexts win "
                         "at the ~12 workers/shard an 8-rank node affords "
                         "(38k req/s, 5.8 ms added)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path "
                         "produced in its last step (response bodies, "
                         "per-step gateway accounting) as DIR/<name>.npy; "
                         "native harness only")
    ap.add_argument("--no-pin", action="store_true",
                    help="leave the CPU affinity alone (default: confine "
                         "the harness to one NUMA node, see "
                         "_pin_to_numa_node)")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements: the warm "
                         "direct-to-upstream latency baseline "
                         "(p50_direct_ms, p50_added_latency_ms) and, on "
                         "multi-rank runs, the state-sync tick timing")
    args = ap.parse_args()
    if args.dump_outputs and not (args.front == "fast"
                                  and args.harness == "native"):
        ap.error("--dump-outputs needs --front fast --harness native")

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    use_gpu = torch.cuda.is_available()
    cpu_affinity = None
    if not args.no_pin:
        cpu_affinity = _pin_to_numa_node(
            _gpu_device(local_rank) if use_gpu and not args.no_gpu else None)
    if world > 1:
        backend = "nccl" if use_gpu else "gloo"
        # AIGW_BENCH_BACKEND=gloo lets a multi-rank run share ONE GPU
        # (RCCL refuses two ranks on a device) — used to rehearse the
        # torchrun + fast-front + statesync + GPU-admission combination
        # on a 1-GPU box before the driver's real 8-GPU scale run
        backend = os.environ.get("AIGW_BENCH_BACKEND", backend)
        if use_gpu:
            torch.cuda.set_device(_gpu_device(local_rank))
        torch.distributed.init_process_group(backend)

    fast_mode = args.front == "fast"

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    front = None
    native = False
    up_procs: list = []
    if fast_mode and args.harness == "native":
        try:
            row, elapsed, workers, front = run_native_bench(
                args, rank, world, local_rank, use_gpu and not args.no_gpu,
                barrier_sync,
            )
            results = [row]
            native = True
        except ImportError:
            if args.dump_outputs:
                raise
            fast_mode = False
    elif fast_mode:
        try:
            front, go, out_q, procs, up_procs, workers = run_fast_mode(
                args, rank, world, local_rank, use_gpu and not args.no_gpu
            )
        except ImportError:
            fast_mode = False
    if not fast_mode:
        workers = args.workers
        if workers <= 0:
            cores = os.cpu_count() or 8
            # measured knee on the 256-core MI355X box: throughput peaks at
            # ~12-16 workers/shard (14.1k req/s @16) and collapses by 32
            # (profiles/r01 bench_wsweep); ~3 cores per worker keeps headroom
            # when 8 ranks share the node
            workers = max(1, min(12, cores // (3 * max(world, 1))))

        gpu_socket = None
        gpu_host_state = None
        if use_gpu and args.gpu_service:
            gpu_socket = f"/tmp/aigw-gpu-{rank}-{os.getpid()}.sock"
            gpu_host_state = _start_gpu_host(gpu_socket, local_rank, args.gpu_window)
        args.gpu_socket = gpu_socket

        ctx = mp.get_context("spawn")
        ready_evts = [ctx.Event() for _ in range(workers)]
        go = ctx.Event()
        out_q = ctx.Queue()
        procs = [
            ctx.Process(target=worker_entry, args=(args, local_rank, ready_evts[i], go, out_q))
            for i in range(workers)
        ]
        for p in procs:
            p.start()
        for ev in ready_evts:
            if not ev.wait(timeout=600):
                for p in procs:
                    p.terminate()
                raise RuntimeError("bench worker failed to become ready")

    if not native:
        barrier_sync()
        t0 = time.perf_counter()
        go.set()
        results = [out_q.get(timeout=600) for _ in range(workers)]
        # closing bracket: all GPU work retired before the clock stops
        if use_gpu:
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        barrier_sync()
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
        for p in up_procs:
            p.terminate()

    statesync_tick_us = None
    if world > 1 and args.full:
        # demonstrate the RCCL-synced rate-limit counters on the same
        # communicator the scale bench uses (BASELINE config: "RCCL-synced
        # rate-limit counters"): a fixed number of fused all-reduce ticks
        # per rank, timed. Deterministic tick count keeps the collective
        # sequence identical across ranks (no timer-driven ticks racing
        # the final all-reduce).
        from aigw.parallel import StateSync

        if native and front is not None:
            # sync the NATIVE front's real rate counters — the serving run
            # just charged them with every timed request's token usage
            from aigw.parallel import FastLimiterBridge

            sync = StateSync(FastLimiterBridge(front.fast, ["node-token-budget"]))
        else:
            from aigw.filterapi import RuntimeConfig as _RC
            from aigw.filterapi import load_config as _lc
            from aigw.ratelimit import RateLimiter

            lim = RateLimiter(_RC(_lc(gateway_config(9))).rate_limits)
            lim.check({})  # touch the bucket so deltas exist
            sync = StateSync(lim)
        sync.tick_sync()  # warm (drains the serving run's pending deltas)
        ts0 = time.perf_counter()
        for _ in range(20):
            sync.tick_sync()
        statesync_tick_us = (time.perf_counter() - ts0) / 20 * 1e6
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        if torch.distributed.get_backend() == "nccl":
            t = t.cuda()
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed_max = float(t.cpu().item())
    else:
        elapsed_max = elapsed

    total_requests = sum(r["requests"] for r in results) * world
    value = total_requests / elapsed_max
    p50 = statistics.median(r["p50"] for r in results)
    p99 = max(r["p99"] for r in results)
    p50_direct = (statistics.median(r["p50_direct"] for r in results)
                  if args.full else None)

    if rank == 0:
        out = {
            "metric": "req/sec (whole node) + p50 added latency, OpenAI chat/completions 4k-token body",
            "value": round(value, 2),
            "unit": "req/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": "aigw standalone: OpenAI /v1/chat/completions -> mock upstream (examples/basic)",
                "global_batch": args.batch * workers * world,
                "waves_per_step": args.waves,
                "seq_len": args.tokens,
                "parallelism": f"dp{world}",
                "front": "fast" if fast_mode else "lean",
                "streamed": bool(getattr(args, "stream", False)) or None,
                "workers_per_shard": workers,
                "cpu_affinity": cpu_affinity,
                "p50_ms": round(p50, 3),
                "p99_ms": round(p99, 3),
                "p50_direct_ms": round(p50_direct, 3) if args.full else None,
                "p50_added_latency_ms": (round(p50 - p50_direct, 3)
                                         if args.full else None),
                "gpu_token_accounting": use_gpu,
                "gpu_admission": (
                    dict(zip(("batches", "texts", "time_us", "max_us",
                              "errors", "pack_us", "submit_us", "wait_us",
                              "fulfill_us"),
                             front.fast.gpu_direct_stats()))
                    if fast_mode and front is not None else None
                ),
                "statesync_tick_us": round(statesync_tick_us, 1) if statesync_tick_us else None,
                "semantic_cache_payload_pool": args.cache_payloads or None,
                "fast_cache_stats": (
                    {k: front.stats()[k] for k in ("cache_hits", "cache_misses")}
                    if fast_mode and front is not None and args.cache_payloads
                    else None
                ),
            },
        }
        print(json.dumps(out))

    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
