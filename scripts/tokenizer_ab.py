"""Parent (two copies, A and A') against this tree: psam_fps / psam_knn, three libraries in one process, device-event times.
    python scripts/tokenizer_ab.py PARENT_COPY_1.so PARENT_COPY_2.so point_sam_amd/csrc/libpointsam_hip.so   (TOK_AB_SHARED=1: one workspace and one pair of outputs for all three)
    Prints the table as markdown."""
import ctypes, os, statistics, sys
import torch

ROUNDS, WARM = 20, 2
SHARED = os.environ.get('TOK_AB_SHARED') == '1'
libs = []
for p in sys.argv[1:4]:
    L = ctypes.CDLL(os.path.abspath(p))
    L.psam_fps_workspace_bytes.restype = ctypes.c_size_t
    L.psam_fps_workspace_bytes.argtypes = [ctypes.c_int32] * 3
    L.psam_fps.restype = ctypes.c_int32
    L.psam_fps.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.psam_knn.restype = ctypes.c_int32
    L.psam_knn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_void_p, ctypes.c_void_p]
    for f in ("psam_fps_set_cooperative", "psam_fps_set_pruning", "psam_knn_force_band"):
        getattr(L, f).argtypes = [ctypes.c_int32]; getattr(L, f).restype = None
    for f in ("psam_fps_last_instance", "psam_knn_last_instance"):
        getattr(L, f).restype = ctypes.c_int32
    libs.append(L)
NAMES = ("A", "A'", "new")
dev = torch.device("cuda")


def cloud(B, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True) * (1.0 + 0.3 * torch.sin(3.0 * v[..., :1]))      # a bumpy closed surface
    return v.to(dev).contiguous()


def timed(fns):
    """fns: one callable per library.  Returns per-library lists of ms."""
    ms = [[] for _ in fns]
    for r in range(WARM + ROUNDS):
        order = [(r + i) % len(fns) for i in range(len(fns))]
        for i in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fns[i](); b.record(); b.synchronize()
            if r >= WARM:
                ms[i].append(a.elapsed_time(b))
    return ms


rows = []


def report(label, inst, ms):
    med = [statistics.median(m) for m in ms]
    spread, diff = abs(med[0] - med[1]), med[2] - med[0]
    margin = max(spread, 0.005 * med[0])
    cell = lambda m: "%.4f [%.4f … %.4f]" % (statistics.median(m), min(m), max(m))
    rows.append("| `%s` | %s | %s | %s | %s | %.4f | %+.4f | %.4f | %s |" % (label, inst, cell(ms[0]), cell(ms[1]), cell(ms[2]), spread, diff, margin, "yes" if abs(diff) <= margin else "NO"))
    print(rows[-1], flush=True)


def fps_case(B, N, G, coop, prune):
    x = cloud(B, N, 1000 + N % 997 + B)
    outs, fns, inst = [], [], None
    for L in libs:
        L.psam_fps_set_cooperative(coop); L.psam_fps_set_pruning(prune)
        wsb = L.psam_fps_workspace_bytes(B, N, G)
        ws = torch.empty(wsb + 64, dtype=torch.uint8, device=dev)
        idx = torch.full((B, G), -1, dtype=torch.int64, device=dev)
        ctr = torch.full((B, G, 3), -7.25, dtype=torch.float32, device=dev)
        call = (lambda L=L, ws=ws, idx=idx, ctr=ctr, wsb=wsb: L.psam_fps(x.data_ptr(), B, N, G, idx.data_ptr(), ctr.data_ptr(), ws.data_ptr(), wsb, None))
        rc = call(); torch.cuda.synchronize()
        assert rc == 0, rc
        inst = L.psam_fps_last_instance() if inst is None else inst
        assert L.psam_fps_last_instance() == inst
        outs.append((idx, ctr, ws)); fns.append(call)
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1].view(torch.int32), outs[0][1].view(torch.int32)), "libraries disagree"
    assert int(outs[0][0].min()) >= 0
    if SHARED:      # time all three on ONE workspace and ONE pair of outputs: the address of the key slots decides which channel the hand-over polls
        idx, ctr, ws = outs[0]
        wsb = libs[0].psam_fps_workspace_bytes(B, N, G)
        fns = [(lambda L=L: L.psam_fps(x.data_ptr(), B, N, G, idx.data_ptr(), ctr.data_ptr(), ws.data_ptr(), wsb, None)) for L in libs]
    report("psam_fps (%d, %d, %d)%s%s" % (B, N, G, "" if coop == 1 else " coop=%d" % coop, "" if prune else " prune=0"), "fps %d" % inst, timed(fns))
    return x, outs[0][1]


def knn_case(B, G, N, K, band, x, ctr):
    outs, fns = [], []
    for L in libs:
        L.psam_knn_force_band(band)
        idx = torch.full((B, G, K), -1, dtype=torch.int64, device=dev)
        call = (lambda L=L, idx=idx: L.psam_knn(ctr.data_ptr(), x.data_ptr(), B, G, N, K, idx.data_ptr(), None))
        rc = call(); torch.cuda.synchronize()
        assert rc == 0 and L.psam_knn_last_instance() == band
        outs.append(idx); fns.append(call)
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "libraries disagree"
    assert int(outs[0].min()) >= 0
    report("psam_knn (%d, %d, %d, %d)%s" % (B, G, N, K, "" if band else " band=0"), "knn %d" % band, timed(fns))


rows.append("| call (B, N, G) / (B, G, N, K) | instance | parent (A) | parent (A') | this tree | A/A' spread | this tree − A | margin | within |\n|---|---|---|---|---|---|---|---|---|")
print(rows[0])
x1, c1 = fps_case(8, 32768, 512, 1, 1)
x2, c2 = fps_case(1, 131072, 2048, 1, 1)
fps_case(1, 32768, 512, 1, 1)
knn_case(8, 512, 32768, 64, 1, x1, c1)
knn_case(1, 2048, 131072, 256, 1, x2, c2)
# the instances the default dispatch does not reach at those sizes
fps_case(1, 524288, 512, 1, 1)
fps_case(1, 32768, 512, 1, 0)
fps_case(1, 131072, 2048, 1, 0)
fps_case(1, 524288, 512, 1, 0)
if not SHARED:
    for N in (8192, 12288, 16384, 20480):
        fps_case(8, N, 256, 0, 1)
    fps_case(1, 65536, 256, 0, 1)
knn_case(8, 512, 32768, 64, 0, x1, c1)
knn_case(1, 2048, 131072, 256, 0, x2, c2)
print("done")
