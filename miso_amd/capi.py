"""ctypes binding of libmiso_amd.so (include/miso_amd.h).

This is the only way Python reaches the sampler: there is no Python or CPU implementation of
the path behind it.  Importing works without a GPU (so the symbol table can be checked);
every sampler call raises ``InternalError`` when no HIP device is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MISO_AMD_LIB", os.path.join(_HERE, "libmiso_amd.so"))

MISO_SUCCESS, MISO_FAILURE, MISO_ENOMEM, MISO_EINVAL = 0, 1, 2, 4
MISO_UNIMPLEMENTED, MISO_EINTERNAL, MISO_ENODEVICE = 12, 38, 60
MISO_MAX_ISOFORMS = 256     # include/miso_amd.h

# pysplicing/pysplicing/__init__.py:2-13
MISO_START_AUTO, MISO_START_UNIFORM, MISO_START_RANDOM, MISO_START_GIVEN, MISO_START_LINEAR = range(5)
MISO_STOP_FIXEDNO, MISO_STOP_CONVERGENT_MEAN = 0, 1
MISO_ALGO_REASSIGN, MISO_ALGO_MARGINAL, MISO_ALGO_CLASSES = 0, 1, 2


class InternalError(Exception):
    """pysplicing.InternalError (pysplicing.c:699-702)."""


class RunData(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("noIso", "noIters", "maxIters", "noBurnIn", "noLag",
                                       "noAccepted", "noRejected", "noChains", "noSamples")]


class Params(C.Structure):
    _fields_ = [("paired", C.c_int), ("readLength", C.c_int), ("overHang", C.c_int),
                ("noChains", C.c_int), ("noIterations", C.c_int), ("maxIterations", C.c_int),
                ("noBurnIn", C.c_int), ("noLag", C.c_int), ("algorithm", C.c_int),
                ("start", C.c_int), ("stop", C.c_int), ("normalMean", C.c_double),
                ("normalVar", C.c_double), ("numDevs", C.c_double),
                ("want_counts_trace", C.c_int), ("device_match", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("waves", C.c_double), ("trips", C.c_double),
                ("iterations", C.c_double), ("chains", C.c_double), ("words", C.c_double)]


_lib = None


def lib():
    """Load libmiso_amd.so; fail loudly if the HIP extension was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "miso_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as "
                "g; g.build()'` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.miso_last_error.restype = C.c_char_p
        _lib.miso_strerror.restype = C.c_char_p
        _lib.miso_batch_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32]
        _lib.miso_batch_run.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32]
        _lib.miso_batch_summarize.argtypes = [C.c_void_p, C.c_double]
        _lib.miso_batch_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    return _lib


def check(rc):
    """Raise like pyerror.c:27-44: MemoryError / NotImplementedError / InternalError."""
    if rc == MISO_SUCCESS:
        return
    msg = lib().miso_last_error().decode(errors="replace")
    if rc == MISO_ENOMEM:
        raise MemoryError(msg)
    if rc == MISO_UNIMPLEMENTED:
        raise NotImplementedError(msg)
    raise InternalError(msg)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _cigs(cigars):
    arr = (C.c_char_p * max(len(cigars), 1))()
    for i, c in enumerate(cigars):
        arr[i] = c if isinstance(c, bytes) else c.encode()
    return arr


def contract_version():
    """include/miso_philox.h MISO_CONTRACT_VERSION of the loaded library (no device needed)."""
    return int(lib().miso_contract_version())


def device_count():
    n = C.c_int(0)
    check(lib().miso_device_count(C.byref(n)))
    return n.value


def set_device(d):
    check(lib().miso_set_device(int(d)))


def usable_threads():
    """Host threads worth starting: the affinity mask capped by the cgroup CPU quota, at most 64 (miso_usable_threads)."""
    return max(1, int(lib().miso_usable_threads()))


class Gene:
    """One gene: exons as (start, end) 1-based inclusive, isoforms as tuples of exon indices
    (py2c_gene.py:10-21 builds exactly these for the reference's createGene)."""

    def __init__(self, exons, isoforms, id="insilicogene", seqid="seq1", source="protein_coding",
                 strand=2):
        ex = np.asarray(exons, dtype=np.int32).reshape(-1)
        flat = []
        for iso in isoforms:
            flat.extend(int(e) for e in iso)
            flat.append(-1)
        flat = np.asarray(flat, dtype=np.int32)
        h = C.c_void_p()
        check(lib().miso_create_gene(_p(ex), len(ex) // 2, _p(flat), len(flat), id.encode(),
                                     seqid.encode(), source.encode(), int(strand), C.byref(h)))
        self.handle = h

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h and _lib is not None:
            _lib.miso_gene_destroy(h)

    @property
    def noiso(self):
        n = C.c_int(0)
        check(lib().miso_gene_noiso(self.handle, C.byref(n)))
        return n.value

    def isolength(self):
        out = np.zeros(self.noiso, np.int32)
        check(lib().miso_gene_isolength(self.handle, _p(out)))
        return out

    def assignment_matrix(self, read_len, overhang=1, max_cols=4096):
        """The gene's possible read classes (assignment.c:90-276): ncls x K, a class per row (include/miso_amd.h)."""
        K = self.noiso
        m = np.zeros(K * max_cols)
        n = C.c_int(0)
        check(lib().miso_gene_assignment_matrix(self.handle, int(read_len), int(overhang), _p(m), max_cols, C.byref(n)))
        return m[:K * n.value].reshape(n.value, K).copy()

    def match_iso(self, pos, cigars, read_len, overhang=1):
        pos = np.asarray(pos, dtype=np.int32)
        m = np.zeros((max(len(pos), 1), self.noiso))
        check(lib().miso_match_iso(self.handle, _p(pos), _cigs(cigars), len(pos), overhang,
                                   read_len, _p(m)))
        return m[:len(pos)]

    def match_iso_paired(self, pos, cigars, read_len, mean, var, num_devs=4.0, overhang=1):
        pos = np.asarray(pos, dtype=np.int32)
        n = len(pos) // 2
        m = np.zeros((max(n, 1), self.noiso))
        fl = np.zeros((max(n, 1), self.noiso), np.int32)
        check(lib().miso_match_iso_paired(self.handle, _p(pos), _cigs(cigars), len(pos), read_len,
                                          overhang, C.c_double(mean), C.c_double(var),
                                          C.c_double(num_devs), _p(m), _p(fl)))
        return m[:n], fl[:n]


class EventResult:
    def __init__(self, samples, loglik, templates, counts, assignment, rundata, counts_hash,
                 counts_trace):
        self.samples = samples              # [S, K]
        self.loglik = loglik                # [S]
        self.class_templates = templates    # [ncls, K]
        self.class_counts = counts          # [ncls]
        self.assignment = assignment        # [N]
        self.rundata = rundata              # RunData
        self.counts_hash = counts_hash      # [C] uint64
        self.counts_trace = counts_trace    # [(M+1), C, K] or None

    def as_tuple(self):
        """The 6-tuple pysplicing.MISO returns (pysplicing.c:112-130, pyconvert.c:172-181)."""
        rd = self.rundata
        K = self.samples.shape[1] if self.samples.ndim == 2 else 0
        return (tuple(tuple(float(v) for v in self.samples[:, k]) for k in range(K)),
                tuple(float(v) for v in self.loglik),
                tuple(tuple(float(v) for v in row) for row in self.class_templates),
                tuple(float(v) for v in self.class_counts),
                tuple(int(v) for v in self.assignment),
                (rd.noIso, rd.noIters, rd.noBurnIn, rd.noLag, rd.noAccepted, rd.noRejected))


# ---- the posterior predictive model check (include/miso_amd.h miso_model_check) ----
FIT_STATUS = ("ok", "no_gene", "no_reads", "too_many_classes", "no_rows")


class ModelFit:
    """One event's model check: status (a FIT_STATUS name); the class table pattern / m / n (class order = the assignment
    matrix's columns), num_reads = sum n, num_off_model; rows, bad_rows, exceed, sum_obs, sum_rep; per class expected, ge, le.
    pvalue = exceed / rows.  Everything but the table is zero unless status == "ok"."""

    def __init__(self, status, pattern, m, n, num_reads, num_off_model, rows, bad_rows, exceed, sum_obs, sum_rep, expected,
                 ge, le):
        self.status, self.pattern, self.m, self.n = status, pattern, m, n
        self.num_reads, self.num_off_model = int(num_reads), int(num_off_model)
        self.rows, self.bad_rows, self.exceed = int(rows), int(bad_rows), int(exceed)
        self.sum_obs, self.sum_rep = float(sum_obs), float(sum_rep)
        self.expected, self.ge, self.le = expected, ge, le

    @property
    def ok(self):
        return self.status == "ok"

    @property
    def pvalue(self):
        return self.exceed / self.rows if self.ok else float("nan")


def model_check(K, pattern, m, n, samples, event_id=None, seed=0, device=0):
    """miso_model_check on caller-given tables: per event e, K[e] isoforms, the classes pattern[e] / m[e] / n[e] (sequences of
    equal length) and samples[e], an array [S, K[e]] of posterior rows.  Returns ([ModelFit], kernel_ms)."""
    L = lib()
    ne = len(K)
    Ks = np.asarray(K, dtype=np.int32)
    Cs = np.asarray([len(x) for x in pattern], dtype=np.int32)
    coff = np.concatenate([[0], np.cumsum(Cs, dtype=np.int64)]).astype(np.int64)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in xs] + [np.zeros(1, dt)]))
    pat, mm, nn = cat(pattern, np.uint64), cat(m, np.int64), cat(n, np.int32)
    rows = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, int(k)) for x, k in zip(samples, Ks)]
    Ss = np.asarray([r.shape[0] for r in rows], dtype=np.int32)
    soff = np.concatenate([[0], np.cumsum([r.size for r in rows], dtype=np.int64)]).astype(np.uint64)
    flat = cat(rows, np.float64)
    ids = np.arange(ne, dtype=np.uint32) if event_id is None else np.asarray(event_id, dtype=np.uint32)
    nc = int(coff[-1]) + 1
    st, ro, ba, ex = (np.zeros(max(ne, 1), np.int32) for _ in range(4))
    so, sr = np.zeros(max(ne, 1)), np.zeros(max(ne, 1))
    exp, ge, le = np.zeros(nc), np.zeros(nc, np.int32), np.zeros(nc, np.int32)
    ms = C.c_float(0)
    check(L.miso_model_check(int(device), ne, _p(Ks), _p(Cs), _p(coff), _p(pat), _p(mm), _p(nn), _p(soff[:-1].copy()), _p(Ss),
                             _p(ids), _p(flat), C.c_uint64(int(soff[-1])), C.c_uint64(int(seed)), _p(st), _p(ro), _p(ba), _p(ex),
                             _p(so), _p(sr), _p(exp), _p(ge), _p(le), C.byref(ms)))
    out = []
    for e in range(ne):
        a, b = int(coff[e]), int(coff[e + 1])
        out.append(ModelFit(FIT_STATUS[st[e]], pat[a:b], mm[a:b], nn[a:b], int(nn[a:b].sum()), 0, ro[e], ba[e], ex[e], so[e],
                            sr[e], exp[a:b], ge[a:b], le[a:b]))
    return out, ms.value


class Batch:
    """Many events, one launch (miso_batch_* in include/miso_amd.h)."""

    def __init__(self, read_len, iters=5000, burn=500, lag=10, chains=6, overhang=1, paired=False,
                 mean=0.0, var=0.0, num_devs=4.0, start=MISO_START_AUTO, stop=MISO_STOP_FIXEDNO,
                 algo=MISO_ALGO_REASSIGN, max_iters=100000, counts_trace=False, device_match=False,
                 collapsed=False, exact=False, exact_paired=False, model_check=False):
        """collapsed (single-end): the two-isoform events draw their assignment COUNTS directly (one exact binomial
        per iteration instead of one uniform per read; miso_batch_set_collapsed in include/miso_amd.h).
        exact (single-end, algo = REASSIGN): the eligible two-isoform events run no chain, their samples are independent
        draws from the posterior of psi itself, tabulated once per event (miso_batch_set_exact in include/miso_amd.h).
        exact_paired (paired-end, algo = REASSIGN): the same for the eligible paired-end two-isoform events, a switch of its
        own (miso_batch_set_exact_paired in include/miso_amd.h).
        model_check (single-end, overhang <= 1): every event added with its gene keeps the gene's class table for the
        posterior predictive check, model_check() (miso_batch_set_model_check in include/miso_amd.h)."""
        self.params = Params(int(paired), read_len, overhang, chains, iters, max_iters, burn, lag,
                             algo, start, stop, mean, var, num_devs, int(counts_trace),
                             int(device_match))
        self.handle = C.c_void_p()
        check(lib().miso_batch_create(C.byref(self.params), C.byref(self.handle)))
        self.collapsed = int(collapsed)     # True / 1: two-isoform events; 2: events of any isoform count
        if collapsed:
            check(lib().miso_batch_set_collapsed(self.handle, int(collapsed)))
        self.exact = bool(exact)
        if exact:
            check(lib().miso_batch_set_exact(self.handle, 1))
        self.exact_paired = bool(exact_paired)
        if exact_paired:
            check(lib().miso_batch_set_exact_paired(self.handle, 1))
        self.model_check_on = bool(model_check)
        if model_check:
            check(lib().miso_batch_set_model_check(self.handle, 1))

    def set_exact_paired(self, on=True):
        """Switch the paired-end exact-posterior mode on or off, also after the upload: the next launch makes its lists anew
        (miso_batch_set_exact_paired)."""
        check(lib().miso_batch_set_exact_paired(self.handle, int(bool(on))))
        self.exact_paired = bool(on)

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h and _lib is not None:
            _lib.miso_batch_destroy(h)

    def add_event(self, gene, pos, cigars, hyper=None):
        pos = np.asarray(pos, dtype=np.int32)
        hy = None if hyper is None else np.asarray(hyper, dtype=np.float64)
        idx = C.c_int(-1)
        check(lib().miso_batch_add_event(self.handle, gene.handle, _p(pos), _cigs(cigars), len(pos),
                                         _p(hy), 0 if hy is None else len(hy), C.byref(idx)))
        return idx.value

    def set_event_id(self, idx, event_id):
        """Pin event idx's id in the Philox counter (default: first_event_id + idx)."""
        check(lib().miso_batch_set_event_id(self.handle, int(idx), C.c_uint32(int(event_id) & 0xFFFFFFFF)))

    def add_problem(self, match, isolen, noexons, fraglen=None, hyper=None):
        """match: [N, K] (C-order) as Gene.match_iso returns it."""
        match = np.ascontiguousarray(match, dtype=np.float64)
        N, K = match.shape
        isolen = np.asarray(isolen, dtype=np.int32)
        noexons = np.asarray(noexons, dtype=np.int32)
        fl = None if fraglen is None else np.ascontiguousarray(fraglen, dtype=np.int32)
        hy = None if hyper is None else np.asarray(hyper, dtype=np.float64)
        idx = C.c_int(-1)
        check(lib().miso_batch_add_problem(self.handle, K, N, _p(match), _p(fl), _p(isolen),
                                           _p(noexons), _p(hy), C.byref(idx)))
        return idx.value

    def add_simulated(self, gene, expression, n_reads, sim_seed, hyper=None):
        """Synthetic reads (miso_simulate_reads) -> add_event, all inside the library."""
        ex = np.asarray(expression, dtype=np.float64)
        hy = None if hyper is None else np.asarray(hyper, dtype=np.float64)
        idx = C.c_int(-1)
        check(lib().miso_batch_add_simulated(self.handle, gene.handle, _p(ex), int(n_reads),
                                             C.c_uint64(sim_seed), _p(hy),
                                             0 if hy is None else len(hy), C.byref(idx)))
        return idx.value

    def __len__(self):
        n = C.c_int(0)
        check(lib().miso_batch_size(self.handle, C.byref(n)))
        return n.value

    def upload(self, device=0):
        check(lib().miso_batch_upload(self.handle, int(device)))

    def launch(self, seed=0, first_event_id=0):
        check(lib().miso_batch_launch(self.handle, int(seed), int(first_event_id)))

    def sync(self):
        ms = C.c_float(0)
        check(lib().miso_batch_sync(self.handle, C.byref(ms)))
        return ms.value

    def download(self):
        check(lib().miso_batch_download(self.handle))

    def run(self, device=0, seed=0, first_event_id=0):
        check(lib().miso_batch_run(self.handle, int(device), int(seed), int(first_event_id)))

    def summarize(self, confidence_level=0.95, as_text=False):
        """Device-side posterior means and credible intervals of every event (no sample download).  as_text: of the
        samples as the `.miso` file hands them to summarize_miso, i.e. after "%.4f" (miso_batch_summarize_as_text)."""
        f = lib().miso_batch_summarize_as_text if as_text else lib().miso_batch_summarize
        f.argtypes = [C.c_void_p, C.c_double]
        check(f(self.handle, C.c_double(confidence_level)))

    def summary(self, i):
        """(mean[K], ci_low[K], ci_high[K]) of event i after summarize()."""
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        m, lo, hi = (np.zeros(K.value) for _ in range(3))
        check(lib().miso_batch_get_summary(self.handle, i, _p(m), _p(lo), _p(hi)))
        return m, lo, hi

    def summarize_isoform_groups(self, groups, confidence_level=0.95, as_text=False):
        """Mean and credible interval of isoform-group columns (miso_batch_summarize_isoform_groups): groups is
        a sequence of (event index, mask), the mask a set of the event's isoform indices as an integer (bit k = isoform k);
        a group's draw is the sum of its isoforms' psi, row by row of the sample pool.  Nothing is stored in the batch."""
        ev, mask = _group_arrays(groups)
        out = np.zeros((len(ev), 3))
        ms = C.c_float(0.0)
        L = lib()
        L.miso_batch_summarize_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int,
                                                          C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
        check(L.miso_batch_summarize_isoform_groups(self.handle, _p(ev), _p(mask), len(ev), C.c_double(confidence_level),
                                                    C.c_int(1 if as_text else 0), _p(out), out.size, C.byref(ms)))
        return IsoformGroupSummary(out, float(ms.value))

    def exact_summary(self, i, confidence_level=0.95):
        """(mean[2], ci_low[2], ci_high[2]) of event i from the exact mode's grid -- no Monte-Carlo error -- after sync();
        None for an event that ran the sampler (miso_batch_get_exact_summary)."""
        m, lo, hi = (np.zeros(2) for _ in range(3))
        was = C.c_int(0)
        check(lib().miso_batch_get_exact_summary(self.handle, int(i), _p(m), _p(lo), _p(hi), C.c_double(confidence_level),
                                                 C.byref(was)))
        return (m, lo, hi) if was.value else None

    def summaries(self, indices, noiso):
        """[(mean[K], ci_low[K], ci_high[K])] of the given events after summarize() -- summary() for many events without its
        per-event allocations (noiso[j] = isoforms of event indices[j], known to the caller from the annotation)."""
        offs = np.concatenate([[0], np.cumsum(np.asarray(noiso, dtype=np.int64))])
        buf = np.zeros((3, int(offs[-1])))
        base = [buf[r].ctypes.data for r in range(3)]
        f = lib().miso_batch_get_summary
        h = self.handle
        for j, i in enumerate(indices):
            o = 8 * int(offs[j])
            check(f(h, int(i), C.c_void_p(base[0] + o), C.c_void_p(base[1] + o), C.c_void_p(base[2] + o)))
        return [(buf[0, offs[j]:offs[j + 1]], buf[1, offs[j]:offs[j + 1]], buf[2, offs[j]:offs[j + 1]]) for j in range(len(indices))]

    def diagnose(self, chains=None):
        """Device-side chain diagnostics of every event (no sample download; miso_batch_diagnose): split
        R-hat, effective sample size, Monte-Carlo standard error of the psi mean.  chains: how many chains the sample
        columns interleave (column s is chain s % chains); None = the batch's own, which a batch of adopted samples
        does not have."""
        check(lib().miso_batch_diagnose(self.handle, C.c_int(0 if chains is None else int(chains))))

    def diagnostics(self, i):
        """(rhat[K], ess[K], mcse[K], lag[K]) of event i after diagnose(); lag as integers."""
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        r, e, m, l = (np.zeros(K.value) for _ in range(4))
        check(lib().miso_batch_get_diagnostics(self.handle, i, _p(r), _p(e), _p(m), _p(l)))
        return r, e, m, l.astype(np.int64)

    def diagnostics_many(self, indices, noiso):
        """[(rhat[K], ess[K], mcse[K], lag[K])] of the given events after diagnose(): diagnostics() for many events, as
        summaries() is summary()'s."""
        offs = np.concatenate([[0], np.cumsum(np.asarray(noiso, dtype=np.int64))])
        buf = np.zeros((4, int(offs[-1])))
        base = [buf[r].ctypes.data for r in range(4)]
        f = lib().miso_batch_get_diagnostics
        h = self.handle
        for j, i in enumerate(indices):
            o = 8 * int(offs[j])
            check(f(h, int(i), *(C.c_void_p(base[r] + o) for r in range(4))))
        lag = buf[3].astype(np.int64)
        return [(buf[0, offs[j]:offs[j + 1]], buf[1, offs[j]:offs[j + 1]], buf[2, offs[j]:offs[j + 1]], lag[offs[j]:offs[j + 1]])
                for j in range(len(indices))]

    def model_check_table(self, i):
        """The class table of event i of a Batch(model_check=True), on the host (miso_batch_model_check_table): a dict of
        status (FIT_STATUS name), pattern (uint64[C], bit k = isoform k), m (int64[C] start positions), n (int32[C] reads),
        num_reads (their sum) and num_off_model (reads whose non-empty pattern is no class)."""
        L = lib()
        st, nc, nr, no = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        check(L.miso_batch_model_check_table(self.handle, int(i), 0, C.byref(st), C.byref(nc), None, None, None, C.byref(nr),
                                             C.byref(no)))
        pat, m, n = np.zeros(nc.value, np.uint64), np.zeros(nc.value, np.int64), np.zeros(nc.value, np.int32)
        check(L.miso_batch_model_check_table(self.handle, int(i), nc.value, None, None, _p(pat), _p(m), _p(n), None, None))
        return {"status": FIT_STATUS[st.value], "pattern": pat, "m": m, "n": n, "num_reads": nr.value, "num_off_model": no.value}

    def model_check(self, seed=0):
        """The posterior predictive model check of every event over the resident samples (miso_batch_model_check, DESIGN.md
        22); it only reads.  Results: model_fit(i) / model_fit_many(indices)."""
        check(lib().miso_batch_model_check(self.handle, C.c_uint64(int(seed))))

    def model_fit(self, i):
        """ModelFit of event i after model_check(), its class table included."""
        return self.model_fit_many([i])[0]

    def model_fit_many(self, indices):
        """[ModelFit] of the given events after model_check(): model_fit() for many events."""
        L = lib()
        h = self.handle
        out = []
        st, rows, bad, exc = C.c_int(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        so, sr = C.c_double(0), C.c_double(0)
        for i in indices:
            t = self.model_check_table(int(i))
            nc = len(t["n"])
            exp, ge, le = np.zeros(nc), np.zeros(nc, np.int32), np.zeros(nc, np.int32)
            check(L.miso_batch_get_model_check(h, int(i), nc, C.byref(st), C.byref(rows), C.byref(bad), C.byref(exc),
                                               C.byref(so), C.byref(sr), _p(exp), _p(ge), _p(le)))
            out.append(ModelFit(FIT_STATUS[st.value], t["pattern"], t["m"], t["n"], t["num_reads"], t["num_off_model"],
                                rows.value, bad.value, exc.value, so.value, sr.value, exp, ge, le))
        return out

    def model_check_ms(self):
        """Kernel time of the last model_check() of this batch (HIP events), ms."""
        a = C.c_float(0)
        check(lib().miso_batch_model_check_ms(self.handle, C.byref(a)))
        return a.value

    def pass_ms(self):
        """(summarize_ms, diagnose_ms): kernel time of the last summarize() and diagnose() of this batch (HIP events)."""
        a, b = C.c_float(0), C.c_float(0)
        check(lib().miso_batch_pass_ms(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def diagnose_rank(self, chains=None, confidence_level=0.95):
        """Device-side rank-normalised chain diagnostics of every event (miso_batch_diagnose_rank): bulk
        and folded split R-hat, bulk effective sample size, and the effective sample size of the two bounds of the
        `confidence_level` credible interval.  chains as in diagnose().  Refused for the whole batch when the used
        draws of a column exceed 8192, the chains 512, or the draws are too few for the interval."""
        check(lib().miso_batch_diagnose_rank(self.handle, C.c_int(0 if chains is None else int(chains)),
                                             C.c_double(confidence_level)))

    def rank_diagnostics(self, i):
        """(rhat_bulk[K], rhat_fold[K], ess_bulk[K], ess_ci_low[K], ess_ci_high[K], distinct[K]) of event i after
        diagnose_rank(); distinct as integers."""
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        cols = [np.zeros(K.value) for _ in range(6)]
        check(lib().miso_batch_get_rank_diagnostics(self.handle, i, *(_p(c) for c in cols)))
        return tuple(cols[:5]) + (cols[5].astype(np.int64),)

    def rank_diagnostics_many(self, indices, noiso):
        """[(rhat_bulk[K], rhat_fold[K], ess_bulk[K], ess_ci_low[K], ess_ci_high[K], distinct[K])] of the given events after
        diagnose_rank(): rank_diagnostics() for many events, as diagnostics_many() is diagnostics()'s."""
        offs = np.concatenate([[0], np.cumsum(np.asarray(noiso, dtype=np.int64))])
        buf = np.zeros((6, int(offs[-1])))
        base = [buf[r].ctypes.data for r in range(6)]
        f = lib().miso_batch_get_rank_diagnostics
        h = self.handle
        for j, i in enumerate(indices):
            o = 8 * int(offs[j])
            check(f(h, int(i), *(C.c_void_p(base[r] + o) for r in range(6))))
        distinct = buf[5].astype(np.int64)
        return [tuple(buf[r, offs[j]:offs[j + 1]] for r in range(5)) + (distinct[offs[j]:offs[j + 1]],)
                for j in range(len(indices))]

    def rank_pass_ms(self):
        """Kernel time of the last diagnose_rank() of this batch (HIP events), ms."""
        a = C.c_float(0)
        check(lib().miso_batch_rank_pass_ms(self.handle, C.byref(a)))
        return a.value

    def compare(self, other, smoothing=0.3):
        """Two-sample comparison with `other` (same events, same order) on the device."""
        check(lib().miso_batch_compare(self.handle, other.handle, C.c_double(smoothing)))

    def comparison(self, i):
        """(mean1[K], mean2[K], bayes_factor[K], density_at_0[K]) of event i after compare()."""
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        m1, m2, bf, dens = (np.zeros(K.value) for _ in range(4))
        check(lib().miso_batch_get_comparison(self.handle, i, _p(m1), _p(m2), _p(bf), _p(dens)))
        return m1, m2, bf, dens

    def compare_exact(self, other, z=()):
        """The exact comparison with `other` (same events, same order; both batches exact=True) on the device, without a
        draw: Bayes factor and P(psi_1 - psi_2 <= z) for every z (at most 8, each in (-1, 1)) from the two posteriors'
        tables (miso_batch_compare_exact in include/miso_amd.h)."""
        zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        check(lib().miso_batch_compare_exact(self.handle, other.handle, _p(zz), C.c_int(len(zz))))
        self._exact_nz = len(zz)

    def compare_exact_paired(self, other, z=()):
        """compare_exact() for two paired-end batches that both ran with exact_paired=True: the product of the two
        posteriors is tabulated over both samples' resident pairs (miso_batch_compare_exact_paired in include/miso_amd.h).
        The results take compare_exact()'s place: exact_comparison(i) reads them."""
        zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        check(lib().miso_batch_compare_exact_paired(self.handle, other.handle, _p(zz), C.c_int(len(zz))))
        self._exact_nz = len(zz)

    def exact_comparison(self, i):
        """(mean1, mean2, log_density_at_0, bayes_factor, log10_bayes_factor, cdf[n_z]) of event i after compare_exact() or
        compare_exact_paired(); None when the pair is not exact-comparable (miso_batch_get_exact_comparison)."""
        v = [C.c_double(0.0) for _ in range(5)]
        cdf = np.zeros(getattr(self, "_exact_nz", 0))
        was = C.c_int(0)
        check(lib().miso_batch_get_exact_comparison(self.handle, int(i), *[C.byref(x) for x in v], _p(cdf), C.byref(was)))
        return tuple(x.value for x in v) + (cdf,) if was.value else None

    def exact_delta_quantiles(self, other, probs=(0.5, 0.025, 0.975)):
        """The quantiles of delta psi = psi_1 - psi_2 at `probs` (at most 4, each inside (0, 1)) from the exact CDF, on the
        device and without a draw, of the pairs the stored compare_exact() / compare_exact_paired() with `other` found
        comparable (miso_batch_exact_delta_quantiles in include/miso_amd.h).  The next exact comparison
        discards them."""
        pp = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        check(lib().miso_batch_exact_delta_quantiles(self.handle, other.handle, _p(pp), C.c_int(len(pp))))
        self._exact_np = len(pp)

    def exact_delta(self, i):
        """(quantiles[n_p], cdf_at_0) of event i after exact_delta_quantiles(): the quantiles of psi_1 - psi_2 and
        P(psi_1 - psi_2 <= 0); None when the pair is not exact-comparable (miso_batch_get_exact_delta_quantiles)."""
        q = np.zeros(getattr(self, "_exact_np", 0))
        h0, was = C.c_double(0.0), C.c_int(0)
        check(lib().miso_batch_get_exact_delta_quantiles(self.handle, int(i), _p(q), C.byref(h0), C.byref(was)))
        return (q, h0.value) if was.value else None

    def exact_delta_ms(self):
        """Kernel time of the last exact_delta_quantiles() stored in this batch (HIP events), ms."""
        a = C.c_float(0)
        check(lib().miso_batch_exact_delta_ms(self.handle, C.byref(a)))
        return float(a.value)

    def exact_stats(self, i):
        """(stats7, was_exact) of event i of a launched batch: (n10, n01, n, e0, e1, h0, h1), what the exact posterior of a
        single-end two-isoform event is made of and exact_delta_groups takes; was_exact False for an event the exact mode did
        not take and for every event of a paired-end batch (miso_batch_get_exact_stats)."""
        r = np.zeros(7)
        was = C.c_int(0)
        check(lib().miso_batch_get_exact_stats(self.handle, int(i), _p(r), C.byref(was)))
        return r, bool(was.value)

    def exact_paired_element(self, i):
        """(stats6, m [n_pairs, 2], was_exact) of event i of a launched batch: (n10, n01, A0, A1, h0, h1) and the drawing
        pairs' probabilities in record order, what the exact posterior of a paired-end two-isoform event is made of and
        exact_paired_delta_groups takes; was_exact False (and nothing else filled) for an event the paired exact mode did
        not take and for every event of a single-end batch (miso_batch_get_exact_paired_element)."""
        r = np.zeros(6)
        n, was = C.c_int64(0), C.c_int(0)
        L = lib()
        L.miso_batch_get_exact_paired_element.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                                          C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        check(L.miso_batch_get_exact_paired_element(self.handle, int(i), _p(r), None, 0, C.byref(n), C.byref(was)))
        m = np.zeros((n.value, 2))
        if was.value and n.value:
            check(L.miso_batch_get_exact_paired_element(self.handle, int(i), _p(r), _p(m), n.value, C.byref(n), C.byref(was)))
        return r, m, bool(was.value)

    def compare_pairs(self, other, confidence_level=0.95, thresholds=(0.1, 0.2), as_text=False):
        """The posterior of delta psi = psi_1 - psi_2 over ALL pairs of this batch's draws and `other`'s (same events, same
        order; the sample counts may differ, 8192 per event at most) on the device: median, credible interval and exact
        counts of the S1 * S2 differences (miso_batch_compare_pairs in include/miso_amd.h).  thresholds: at
        most 4, each inside (0, 1).  The results stand beside compare()'s.  as_text: of the draws as the `.miso` files print
        them, "%.4f" (miso_batch_compare_pairs_as_text)."""
        tt = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        f = lib().miso_batch_compare_pairs_as_text if as_text else lib().miso_batch_compare_pairs
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int]
        check(f(self.handle, other.handle, C.c_double(confidence_level), _p(tt), C.c_int(len(tt))))
        self._pairs_nt = len(tt)

    def pair_comparison(self, i):
        """(median[K], ci_low[K], ci_high[K], n_gt0[K], n_lt0[K], n_abs_ge[K, n_tau], finite[K], n_pairs) of event i after
        compare_pairs(): the counts as int64, finite as bool; a probability is count / n_pairs."""
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        nt = getattr(self, "_pairs_nt", 0)
        med, lo, hi = (np.zeros(K.value) for _ in range(3))
        gt, lt = np.zeros(K.value, np.int64), np.zeros(K.value, np.int64)
        ge = np.zeros((K.value, nt), np.int64)
        fin = np.zeros(K.value, np.int32)
        M = C.c_int64(0)
        check(lib().miso_batch_get_pair_comparison(self.handle, int(i), _p(med), _p(lo), _p(hi), _p(gt), _p(lt), _p(ge), _p(fin),
                                                   C.byref(M)))
        return med, lo, hi, gt, lt, ge, fin.astype(bool), int(M.value)

    def compare_pairs_ms(self):
        """Kernel time of the last compare_pairs() stored in this batch (HIP events), ms."""
        a = C.c_float(0)
        check(lib().miso_batch_compare_pairs_ms(self.handle, C.byref(a)))
        return float(a.value)

    def compare_ms(self):
        """(kernel ms of the last compare(), of the last compare_exact() or compare_exact_paired()) stored in this batch"""
        a, b = C.c_float(0), C.c_float(0)
        check(lib().miso_batch_compare_ms(self.handle, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def add_event_aln(self, gene, alnfile, chrom, start, end, strand_rule=0, target_strand=None,
                      read_len=None, min_reads=0, hyper=None):
        """One event straight from an open alignment file (sam_utils.Samfile) -- fetch, pairing and
        filters run natively (miso_batch_add_event_aln).  Returns (event index or -1, reads found)."""
        hy = None if hyper is None else np.asarray(hyper, dtype=np.float64)
        tid = alnfile.gettid(chrom)
        if tid < 0:
            return -1, 0
        idx, n = C.c_int(-1), C.c_int64(0)
        L = lib()
        L.miso_batch_add_event_aln.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                               C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64,
                                               C.c_void_p, C.c_int, C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int)]
        check(L.miso_batch_add_event_aln(self.handle, gene.handle, alnfile._h, tid, int(start),
                                         int(end), int(strand_rule),
                                         ord(target_strand[0]) if target_strand else 0,
                                         int(read_len) if read_len else 0, int(min_reads), _p(hy),
                                         0 if hy is None else len(hy), C.byref(n), C.byref(idx)))
        return idx.value, n.value

    def add_events_aln(self, genes, alnfile, chroms, starts, ends, strand_rule=0, target_strands=None,
                       read_len=None, min_reads=0, threads=0):
        """Many events from one alignment file at once (miso_batch_add_events_aln: reads collected
        and CIGARs parsed on host threads).  Returns (event indices (-1 = not added), reads found)."""
        n = len(genes)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int64)
        tids = np.asarray([alnfile.gettid(c) for c in chroms], dtype=np.int32)
        st = np.asarray(starts, dtype=np.int64)
        en = np.asarray(ends, dtype=np.int64)
        ts = np.asarray([ord(t[0]) if t else 0 for t in (target_strands or [None] * n)], dtype=np.int32)
        gh = (C.c_void_p * n)(*[g.handle for g in genes])
        idx = np.full(n, -1, np.int32)
        cnt = np.zeros(n, np.int64)
        L = lib()
        L.miso_batch_add_events_aln.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        check(L.miso_batch_add_events_aln(self.handle, n, gh, alnfile._h, _p(tids), _p(st), _p(en),
                                          int(strand_rule), _p(ts), int(read_len) if read_len else 0,
                                          int(min_reads), int(threads), _p(cnt), _p(idx)))
        return idx, cnt

    def result_lite(self, i):
        """(class_templates, class_counts, assignment, rundata) of event i -- no sample copy."""
        K, N, ncls = C.c_int(), C.c_int(), C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), C.byref(N), None, C.byref(ncls)))
        ct = np.zeros((max(ncls.value, 1), K.value))
        cc = np.zeros(max(ncls.value, 1))
        ass = np.zeros(max(N.value, 1), np.int32)
        rd = RunData()
        check(lib().miso_batch_get_result(self.handle, i, None, None, _p(ct), _p(cc), _p(ass),
                                          C.byref(rd)))
        return ct[:ncls.value], cc[:ncls.value], ass[:N.value], rd

    def header_fields(self, indices):
        """[(all_unassigned, percent_accept, counts, assigned_counts)] -- the run-dependent header fields of the given
        events as text, formatted natively (include/miso_amd.h miso_batch_header_fields)."""
        n = len(indices)
        if n == 0:
            return []
        idx = np.asarray(indices, dtype=np.int32)
        need = C.c_int64(0)
        cap = 96 * n + 4096
        for _ in range(2):
            buf = C.create_string_buffer(cap)
            check(lib().miso_batch_header_fields(self.handle, n, _p(idx), buf, C.c_int64(cap), C.byref(need)))
            if need.value <= cap:
                break
            cap = need.value
        out = []
        for ln in buf.raw[:need.value - 1].decode().split("\n")[:n]:
            u, pa, counts, assigned = ln.split("\t")
            out.append((u == "1", pa, counts, assigned))
        return out

    def write_miso_files(self, indices, paths, headers, threads=0):
        """The `.miso` files of the given events, rows formatted and written natively."""
        n = len(indices)
        if n == 0:
            return
        idx = np.asarray(indices, dtype=np.int32)
        pa = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        hd = (C.c_char_p * n)(*[h.encode() for h in headers])
        check(lib().miso_batch_write_miso_files(self.handle, n, _p(idx), pa, hd, int(threads)))

    def match_ms(self):
        ms = C.c_float(0)
        check(lib().miso_batch_last_match_ms(self.handle, C.byref(ms)))
        return ms.value

    def device_match_of(self, i):
        """(match [N, K], fraglen [N, K] or None) as the GPU computed them (device_match +
        counts_trace batches, after upload)."""
        K, N = C.c_int(), C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), C.byref(N), None, None))
        m = np.zeros((N.value, K.value))
        fl = np.zeros((N.value, K.value), np.int32) if self.params.paired else None
        check(lib().miso_batch_get_match(self.handle, i, _p(m), _p(fl)))
        return m, fl

    def last_kernels(self):
        buf = C.create_string_buffer(2048)
        check(lib().miso_batch_last_kernels(self.handle, buf, 2048))
        return buf.value.decode()

    def rounds(self):
        """stop=CONVERGENT_MEAN: rounds the last launch took (include/miso_amd.h miso_batch_rounds)"""
        n = C.c_int(0)
        check(lib().miso_batch_rounds(self.handle, C.byref(n)))
        return n.value

    def set_clock_probe(self, on=True):
        """Measure the shader clock of every following launch (include/miso_amd.h miso_batch_set_clock_probe)."""
        check(lib().miso_batch_set_clock_probe(self.handle, int(bool(on))))

    def last_clock(self):
        """(shader clock in GHz, the probe's window in ms) of the last synced launch; (0.0, 0.0) without a valid probe."""
        ghz, ms = C.c_double(0.0), C.c_double(0.0)
        check(lib().miso_batch_last_clock(self.handle, C.byref(ghz), C.byref(ms)))
        return ghz.value, ms.value

    def coop_retries(self):
        """Launches sync() repeated with one workgroup per chain after a chain on several workgroups timed out."""
        n = C.c_int(0)
        check(lib().miso_batch_coop_retries(self.handle, C.byref(n)))
        return n.value

    def launch_stats(self):
        """{"kernels": [{name, waves, trips, iterations, chains, words}], "uniforms": Philox words the
        read loops consume per launch} of the last launch (miso_batch_launch_stats)."""
        n = C.c_int(0)
        cap = 16
        while True:   # (one record per run: a whole-gene batch with size buckets has two dozen; the call reports how many there are)
            arr = (KernelStat * cap)()
            check(lib().miso_batch_launch_stats(self.handle, arr, cap, C.byref(n)))
            if n.value <= cap:
                break
            cap = n.value
        ks = [{"name": arr[i].name.decode(), "waves": arr[i].waves, "trips": arr[i].trips,
               "iterations": arr[i].iterations, "chains": arr[i].chains, "words": arr[i].words}
              for i in range(n.value)]
        return {"kernels": ks, "uniforms": sum(k["words"] * k["iterations"] for k in ks)}

    def placement(self, i):
        """HW_REG_HW_ID of the wavefront that ran each chain of event i (after download)."""
        out = np.zeros(self.params.noChains, np.uint32)
        check(lib().miso_batch_get_placement(self.handle, i, _p(out)))
        return out

    def algorithmic_bytes(self):
        b = C.c_double(0)
        check(lib().miso_batch_algorithmic_bytes(self.handle, C.byref(b)))
        return b.value

    def classes(self, i):
        """(templates [ncls, K], counts [ncls]) of event i: available before any GPU work."""
        K, ncls = C.c_int(), C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, C.byref(ncls)))
        ct = np.zeros((max(ncls.value, 1), K.value))
        cc = np.zeros(max(ncls.value, 1))
        check(lib().miso_batch_get_result(self.handle, i, None, None, _p(ct), _p(cc), None, None))
        return ct[:ncls.value], cc[:ncls.value]

    def result(self, i, trace=False):
        K, N, S, ncls = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), C.byref(N), C.byref(S),
                                          C.byref(ncls)))
        K, N, S, ncls = K.value, N.value, S.value, ncls.value
        samples = np.zeros((max(S, 1), K))
        ll = np.zeros(max(S, 1))
        ct = np.zeros((max(ncls, 1), K))
        cc = np.zeros(max(ncls, 1))
        ass = np.zeros(max(N, 1), np.int32)
        rd = RunData()
        check(lib().miso_batch_get_result(self.handle, i, _p(samples), _p(ll), _p(ct), _p(cc),
                                          _p(ass), C.byref(rd)))
        Cn, M = self.params.noChains, self.params.noIterations
        h = np.zeros(Cn, np.uint64)
        tr = np.zeros((M + 1, Cn, K), np.int32) if trace else None
        check(lib().miso_batch_get_trace(self.handle, i, _p(h), _p(tr)))
        return EventResult(samples[:S], ll[:S], ct[:ncls], cc[:ncls], ass[:N], rd, h, tr)


class SamplesBatch(Batch):
    """Posterior samples produced elsewhere (parsed `.miso` files) on the device: summarize(), summary(i),
    compare(other), comparison(i), diagnose(chains), diagnostics(i), diagnostics_many() as on a sampled batch
    (miso_batch_from_samples), and diagnose_rank(chains), rank_diagnostics(i), rank_diagnostics_many() likewise;
    diagnose() and diagnose_rank() need their `chains` here, the samples carry no chain count."""

    def __init__(self, samples, device=0):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in samples]     # each [S, K]
        n = len(arrs)
        S = arrs[0].shape[0] if n else 1
        if any(a.ndim != 2 or a.shape[0] != S for a in arrs):
            raise ValueError("every event needs the same number of samples")
        K = np.asarray([a.shape[1] for a in arrs], dtype=np.int32)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        self.params = Params(0, 36, 1, 1, S, S, 0, 1, MISO_ALGO_REASSIGN, MISO_START_AUTO, MISO_STOP_FIXEDNO, 0.0, 0.0, 4.0, 0, 0)
        self.handle = C.c_void_p()
        L = lib()
        L.miso_batch_from_samples.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        check(L.miso_batch_from_samples(n, _p(K), int(S), ptrs, int(device), C.byref(self.handle)))

    @classmethod
    def from_text(cls, text, offsets, noiso, n_samples, device=0, chunk_bytes=0):
        """The same batch from the files' TEXT, decoded on the device (miso_batch_from_miso_text): event i's rows are
        text[offsets[i]:offsets[i + 1]] (bytes / uint8 array; what follows a `.miso` file's two header lines).
        `status` (int32 per event, 0 = decoded, else a sum of MISO_TEXT_* bits: its results must not be read) and
        `text_stats` (dict) say how it went."""
        buf = _text_buf(text)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        K = np.ascontiguousarray(noiso, dtype=np.int32)
        n = len(K)
        if len(offs) != n + 1 or (n and (offs[0] < 0 or offs[-1] > len(buf))):
            raise ValueError("offsets must be n_events + 1 positions inside the text")
        self = cls.__new__(cls)
        S = int(n_samples)
        self.params = Params(0, 36, 1, 1, S, S, 0, 1, MISO_ALGO_REASSIGN, MISO_START_AUTO, MISO_STOP_FIXEDNO, 0.0, 0.0, 4.0, 0, 0)
        self.handle = C.c_void_p()
        self.status = np.zeros(max(n, 1), np.int32)
        stats = TextStats()
        L = lib()
        L.miso_batch_from_miso_text.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.POINTER(TextStats)]
        check(L.miso_batch_from_miso_text(n, _p(buf), _p(offs), _p(K), S, int(device), int(chunk_bytes),
                                          C.byref(self.handle), _p(self.status), C.byref(stats)))
        self.status = self.status[:n]
        self.text_stats = stats.as_dict()
        return self

    def samples(self, i):
        """Event i's samples [S, K] as the pool holds them (downloads the pool once)."""
        if not getattr(self, "_downloaded", False):
            check(lib().miso_batch_download(self.handle))
            self._downloaded = True
        K = C.c_int()
        check(lib().miso_batch_event_info(self.handle, i, C.byref(K), None, None, None))
        out = np.zeros((self.params.noIterations, K.value))
        check(lib().miso_batch_get_result(self.handle, i, _p(out), None, None, None, None, None))
        return out


# ---- every pair of two groups of samples (include/miso_amd.h miso_batch_compare_groups) ----
MISO_STAGE_AUTO, MISO_STAGE_BOTH, MISO_STAGE_SMALLER, MISO_STAGE_NONE = 0, 1, 2, 3
STAGING = {"auto": MISO_STAGE_AUTO, "both": MISO_STAGE_BOTH, "smaller": MISO_STAGE_SMALLER, "none": MISO_STAGE_NONE}


class GroupComparison:
    """What compare_groups computed: comparison(i, j, event) is Batch.comparison(event)'s tuple for the pair
    (batches1[i], batches2[j]); `kernel_ms` the kernel's time."""

    def __init__(self, out, n2, noiso, kernel_ms):
        self.noiso = np.asarray(noiso, dtype=np.int64)
        self.offs = np.concatenate([[0], np.cumsum(4 * self.noiso)])
        self.out = out.reshape(-1, n2, int(self.offs[-1]))
        self.kernel_ms = kernel_ms

    def comparison(self, i, j, event):
        """(mean1[K], mean2[K], bayes_factor[K], density_at_0[K]) of `event` for the pair (i, j)."""
        if not 0 <= event < len(self.noiso):
            raise IndexError("event %d of %d" % (event, len(self.noiso)))
        q = self.out[i, j, self.offs[event]:self.offs[event + 1]].reshape(-1, 4)
        return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy(), q[:, 3].copy()


def compare_groups(batches1, batches2, smoothing=0.3, staging="auto", noiso=None):
    """Every pair (batches1[i], batches2[j]) in one device pass: the batches hold the same events in the same order with
    the same number of samples, on one device.  Bit for bit what batches1[i].compare(batches2[j], smoothing) gives.
    staging: which sample columns a workgroup keeps in LDS (`auto`, `both`, `smaller`, `none`).  noiso: the
    events' isoform counts where the caller knows them (else asked of the first batch, event by event)."""
    b1, b2 = list(batches1), list(batches2)
    L = lib()
    L.miso_batch_compare_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                            C.c_int64, C.POINTER(C.c_float)]
    h1 = (C.c_void_p * max(len(b1), 1))(*[b.handle for b in b1])
    h2 = (C.c_void_p * max(len(b2), 1))(*[b.handle for b in b2])
    if noiso is not None:
        noiso = [int(k) for k in noiso]
    else:
        noiso = []
    if not noiso and b1 and len(b1[0]):
        K = C.c_int()
        for e in range(len(b1[0])):
            check(L.miso_batch_event_info(b1[0].handle, e, C.byref(K), None, None, None))
            noiso.append(K.value)
    out = np.zeros(len(b1) * len(b2) * 4 * int(sum(noiso)))
    ms = C.c_float(0.0)
    check(L.miso_batch_compare_groups(h1, len(b1), h2, len(b2), C.c_double(smoothing), STAGING[staging], _p(out),
                                      out.size, C.byref(ms)))
    return GroupComparison(out, len(b2), noiso, float(ms.value))


# ---- delta psi between two pooled groups of samples (include/miso_amd.h miso_batch_compare_pairs_groups) ----
PAIRS_FIXED_WORDS = 6        # csrc/compare_pairs.hpp: median, ci_low, ci_high, n_gt0, n_lt0, finite; then n_abs_ge per threshold
MAX_GROUP_PAIR_DRAWS = 16384


class GroupPairComparison:
    """What compare_pairs_groups computed: pair_comparison(event) is Batch.pair_comparison's tuple for the two pooled groups;
    `kernel_ms` the launches' time, `n_pairs` = M."""

    def __init__(self, out, noiso, n_tau, n_pairs, kernel_ms):
        self.noiso = np.asarray(noiso, dtype=np.int64)
        self.offs = np.concatenate([[0], np.cumsum(self.noiso)])
        self.n_tau = n_tau
        self.out = out.reshape(int(self.offs[-1]), PAIRS_FIXED_WORDS + n_tau)
        self.n_pairs = n_pairs
        self.kernel_ms = kernel_ms

    def pair_comparison(self, event):
        """(median[K], ci_low[K], ci_high[K], n_gt0[K], n_lt0[K], n_abs_ge[K, n_tau], finite[K], n_pairs) of `event`."""
        if not 0 <= event < len(self.noiso):
            raise IndexError("event %d of %d" % (event, len(self.noiso)))
        q = self.out[self.offs[event]:self.offs[event + 1]]
        d = np.ascontiguousarray(q[:, :3]).view(np.float64)
        return (d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy(), q[:, 3].astype(np.int64), q[:, 4].astype(np.int64),
                q[:, PAIRS_FIXED_WORDS:].astype(np.int64), q[:, 5] != 0, self.n_pairs)


def compare_pairs_groups(batches1, batches2, confidence_level=0.95, thresholds=(0.1, 0.2), as_text=False, noiso=None):
    """Batch.compare_pairs for two groups of replicates, pooled: per (event, isoform) the median, credible interval and exact
    counts of ALL differences between the draws of batches1 taken together and those of batches2 taken together
    (DESIGN.md 19a).  The batches are what compare_groups takes: the same events in the same order with the same number of
    samples S, on one device; len(batches) * S is 16384 at most on either side.  Nothing is stored in a batch.
    noiso: the events' isoform counts where the caller knows them."""
    b1, b2 = list(batches1), list(batches2)
    L = lib()
    L.miso_batch_compare_pairs_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    h1 = (C.c_void_p * max(len(b1), 1))(*[b.handle for b in b1])
    h2 = (C.c_void_p * max(len(b2), 1))(*[b.handle for b in b2])
    noiso = [int(k) for k in noiso] if noiso is not None else []
    if not noiso and b1 and len(b1[0]):
        K = C.c_int()
        for e in range(len(b1[0])):
            check(L.miso_batch_event_info(b1[0].handle, e, C.byref(K), None, None, None))
            noiso.append(K.value)
    tt = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.zeros(int(sum(noiso)) * (PAIRS_FIXED_WORDS + len(tt)), np.uint64)
    ms, M = C.c_float(0.0), C.c_int64(0)
    check(L.miso_batch_compare_pairs_groups(h1, len(b1), h2, len(b2), C.c_double(confidence_level), _p(tt), C.c_int(len(tt)),
                                            C.c_int(1 if as_text else 0), _p(out), out.size, C.byref(M), C.byref(ms)))
    return GroupPairComparison(out, noiso, len(tt), int(M.value), float(ms.value))


# ---- part-level psi: isoform-group columns (include/miso_amd.h miso_batch_summarize_isoform_groups) ----
MAX_ISOFORM_GROUP_DRAWS = 8192      # csrc/compare_pairs.hpp PAIRS_MAX_DRAWS: the derived columns live sorted in LDS


def _group_arrays(groups):
    """(event index, mask) pairs as the two arrays the C ABI takes"""
    gs = [(int(e), int(m)) for e, m in groups]
    if any(not 0 <= m < 1 << 64 for _, m in gs):
        raise ValueError("an isoform mask holds 64 bits")
    return (np.asarray([e for e, _ in gs], dtype=np.int32).reshape(-1),
            np.asarray([m for _, m in gs], dtype=np.uint64).reshape(-1))


class IsoformGroupSummary:
    """What Batch.summarize_isoform_groups computed: mean, ci_low, ci_high [n_groups] (three NaN for a group that is not
    finite); summary(g) is one group's triple; `kernel_ms` the launches' time."""

    def __init__(self, out, kernel_ms):
        self.out = out
        self.mean, self.ci_low, self.ci_high = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.out)

    def summary(self, g):
        return float(self.mean[g]), float(self.ci_low[g]), float(self.ci_high[g])


class IsoformGroupPairComparison:
    """What compare_pairs_isoform_groups computed: pair_comparison(g) is group g's (median, ci_low, ci_high, n_gt0, n_lt0,
    n_abs_ge[n_tau], finite, n_pairs), a probability being count / n_pairs; `kernel_ms` the launches' time."""

    def __init__(self, out, n_tau, n_pairs, kernel_ms):
        self.n_tau = n_tau
        self.out = out.reshape(-1, PAIRS_FIXED_WORDS + n_tau)
        self.n_pairs = n_pairs
        self.kernel_ms = kernel_ms

    def __len__(self):
        return len(self.out)

    def pair_comparison(self, g):
        q = self.out[g]
        d = np.ascontiguousarray(q[:3]).view(np.float64)
        return (float(d[0]), float(d[1]), float(d[2]), int(q[3]), int(q[4]), [int(v) for v in q[PAIRS_FIXED_WORDS:]],
                bool(q[5] != 0), self.n_pairs)


def compare_pairs_isoform_groups(batch1, batch2, groups, confidence_level=0.95, thresholds=(0.1, 0.2), as_text=False):
    """Batch.compare_pairs for isoform-group columns: per group (event index, mask) the median, credible interval and exact
    counts of ALL differences between the group's draws in batch1 and in batch2.  The batches as
    Batch.compare_pairs takes them.  Nothing is stored in a batch."""
    ev, mask = _group_arrays(groups)
    tt = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.zeros(len(ev) * (PAIRS_FIXED_WORDS + len(tt)), np.uint64)
    ms, M = C.c_float(0.0), C.c_int64(0)
    L = lib()
    L.miso_batch_compare_pairs_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double,
                                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                                          C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    check(L.miso_batch_compare_pairs_isoform_groups(batch1.handle, batch2.handle, _p(ev), _p(mask), len(ev),
                                                    C.c_double(confidence_level), _p(tt), C.c_int(len(tt)),
                                                    C.c_int(1 if as_text else 0), _p(out), out.size, C.byref(M), C.byref(ms)))
    return IsoformGroupPairComparison(out, len(tt), int(M.value), float(ms.value))


class ExactGroupDelta:
    """What exact_delta_groups / exact_delta_groups_batches computed: `out` [n_events, 2 + n_p + 1 + n_z] (a row the device did
    not write stays NaN), `was_exact` [n_events], `kernel_ms` the launches' time."""

    def __init__(self, out, was_exact, n_p, n_z, kernel_ms):
        self.out, self.was_exact, self.n_p, self.n_z, self.kernel_ms = out, was_exact, n_p, n_z, kernel_ms

    def row(self, event):
        """(mean1, mean2, quantiles[n_p], cdf_at_0, cdf[n_z]) of `event`: the groups' mean posterior means, the quantiles of
        psi_1 - psi_2 pooled over all pairs of replicates, P(delta <= 0) and P(delta <= z); None when the event is not
        comparable."""
        if not 0 <= event < len(self.was_exact):
            raise IndexError("event %d of %d" % (event, len(self.was_exact)))
        if not self.was_exact[event]:
            return None
        r = self.out[event]
        return float(r[0]), float(r[1]), r[2:2 + self.n_p].copy(), float(r[2 + self.n_p]), r[3 + self.n_p:].copy()


def _exact_group_args(probs, z, n_events):
    pp = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    out = np.full((n_events, 2 + len(pp) + 1 + len(zz)), np.nan)
    return pp, zz, out, np.zeros(n_events, np.int32)


def exact_delta_groups(stats1, stats2, probs=(0.5, 0.025, 0.975), z=(), max_events_per_launch=0):
    """Quantiles of delta psi between two groups of replicates from their exact posteriors, pooled over all pairs of
    replicates with equal weights, on the device and without a draw (miso_exact_delta_groups in include/miso_amd.h, DESIGN.md
    20a).  stats_g: [n_events, n_g, 7] rows (n10, n01, n, e0, e1, h0, h1), 1 <= n_g <= 8 -- what Batch.exact_stats returns and
    a `.miso_exact_stats` table holds.  probs: at most 4, inside (0, 1); z: at most 8 points inside (-1, 1)."""
    s1 = np.ascontiguousarray(stats1, dtype=np.float64)
    s2 = np.ascontiguousarray(stats2, dtype=np.float64)
    if s1.ndim != 3 or s2.ndim != 3 or s1.shape[2] != 7 or s2.shape[2] != 7 or s1.shape[0] != s2.shape[0]:
        raise ValueError("stats1, stats2: [n_events, n_replicates, 7] each, with as many events")
    n = s1.shape[0]
    pp, zz, out, was = _exact_group_args(probs, z, n)
    ms = C.c_float(0.0)
    L = lib()
    L.miso_exact_delta_groups.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    check(L.miso_exact_delta_groups(_p(s1), s1.shape[1], _p(s2), s2.shape[1], n, _p(pp), len(pp), _p(zz), len(zz),
                                    int(max_events_per_launch), _p(out), _p(was), C.byref(ms)))
    return ExactGroupDelta(out, was, len(pp), len(zz), float(ms.value))


def _exact_groups_batches(symbol, batches1, batches2, probs, z):
    """the batches' route of either family: the handles of both groups to `symbol` of the library"""
    b1, b2 = list(batches1), list(batches2)
    n = len(b1[0]) if b1 else (len(b2[0]) if b2 else 0)
    pp, zz, out, was = _exact_group_args(probs, z, n)
    ms = C.c_float(0.0)
    fn = getattr(lib(), symbol)
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                   C.c_void_p, C.POINTER(C.c_float)]
    h1 = (C.c_void_p * max(len(b1), 1))(*[b.handle for b in b1])
    h2 = (C.c_void_p * max(len(b2), 1))(*[b.handle for b in b2])
    check(fn(h1, len(b1), h2, len(b2), _p(pp), len(pp), _p(zz), len(zz), _p(out), out.size, _p(was), C.byref(ms)))
    return ExactGroupDelta(out, was, len(pp), len(zz), float(ms.value))


def exact_delta_groups_batches(batches1, batches2, probs=(0.5, 0.025, 0.975), z=()):
    """exact_delta_groups over launched single-end Batch(exact=True) objects that hold the same events in the same order on
    one device (miso_batch_exact_delta_groups): the rows are the batches' exact_stats.  Nothing is stored in a batch."""
    return _exact_groups_batches("miso_batch_exact_delta_groups", batches1, batches2, probs, z)


def exact_paired_delta_groups(group1, group2, probs=(0.5, 0.025, 0.975), z=(), max_events_per_launch=0):
    """exact_delta_groups for PAIRED-END replicates (miso_exact_paired_delta_groups in include/miso_amd.h).
    Each group is a list of 1 .. 8 replicates (stats6 [n_events, 6], pairs), stats6 rows (n10, n01, A0, A1, h0, h1) and
    pairs[i] = the drawing pairs [(m0, m1), ...] of event i, as selftest_exact_paired_delta_quantiles takes one sample --
    what Batch.exact_paired_element returns and a `.miso_exact_pairs` table holds.  All replicates hold the same events in
    the same order."""
    reps = [_pair_lists(st, pairs) for st, pairs in list(group1) + list(group2)]
    n1, n2 = len(group1), len(group2)
    n = len(reps[0][0]) if reps else 0
    if any(len(r[0]) != n for r in reps):
        raise ValueError("every replicate: one row of stats6 and one list of pairs per event, as many events each")
    pp, zz, out, was = _exact_group_args(probs, z, n)
    ms = C.c_float(0.0)
    nb = max(len(reps), 1)
    st = (C.c_void_p * nb)(*[r[0].ctypes.data for r in reps])
    mm = (C.c_void_p * nb)(*[r[1].ctypes.data for r in reps])
    oo = (C.c_void_p * nb)(*[r[2].ctypes.data for r in reps])
    L = lib()
    L.miso_exact_paired_delta_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    check(L.miso_exact_paired_delta_groups(st, mm, oo, n1, n2, n, _p(pp), len(pp), _p(zz), len(zz), int(max_events_per_launch),
                                           _p(out), _p(was), C.byref(ms)))
    return ExactGroupDelta(out, was, len(pp), len(zz), float(ms.value))


def exact_paired_delta_groups_batches(batches1, batches2, probs=(0.5, 0.025, 0.975), z=()):
    """exact_paired_delta_groups over launched paired-end Batch(exact_paired=True) objects that hold the same events in the
    same order on one device (miso_batch_exact_paired_delta_groups): the kernels read the batches' resident pair records.
    Nothing is stored in a batch."""
    return _exact_groups_batches("miso_batch_exact_paired_delta_groups", batches1, batches2, probs, z)


# ---- `.miso` sample text (include/miso_amd.h miso_text_shape, miso_batch_from_miso_text) ----
MISO_TEXT_EPSI, MISO_TEXT_EROW, MISO_TEXT_ESCORE, MISO_TEXT_ECOUNT = 1, 2, 4, 8


class TextStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("chunks", "decoded", "not_decoded", "text_bytes", "sample_bytes")]
                + [(n, C.c_double) for n in ("kernel_ms", "decode_ms", "total_ms")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _text_buf(text):
    if len(text) == 0:
        return np.zeros(1, np.uint8)[:0]
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


def text_shape(text, offsets):
    """(isoforms, non-empty lines) per event body text[offsets[i]:offsets[i + 1]] -- host only, no device needed."""
    buf = _text_buf(text)
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offs) - 1
    if n < 0 or (n and (offs[0] < 0 or offs[-1] > len(buf))):
        raise ValueError("offsets must be n_events + 1 positions inside the text")
    K, rows = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    L = lib()
    L.miso_text_shape.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.miso_text_shape(n, _p(buf), _p(offs), _p(K), _p(rows)))
    return K[:n], rows[:n]


def simulate_reads(gene, expression, n_reads, read_len, sim_seed, mean=0.0, var=0.0, num_devs=4.0):
    """pysplicing.simulateReads / simulatePairedReads (var > 0): returns (isoform, pos, cigars)."""
    ex = np.asarray(expression, dtype=np.float64)
    n = n_reads * (2 if var > 0 else 1)
    stride = 64
    iso = np.zeros(max(n, 1), np.int32)
    pos = np.zeros(max(n, 1), np.int32)
    buf = C.create_string_buffer(max(n, 1) * stride)
    check(lib().miso_simulate_reads(gene.handle, _p(ex), int(n_reads), int(read_len),
                                    C.c_double(mean), C.c_double(var), C.c_double(num_devs),
                                    C.c_uint64(sim_seed), _p(iso), _p(pos), buf, stride))
    raw = buf.raw
    cig = [raw[i * stride:(i + 1) * stride].split(b"\0")[0] for i in range(n)]
    return iso[:n], pos[:n], cig


def selftest_detmath(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    outs = [np.zeros_like(x) for _ in range(4)]
    check(lib().miso_selftest_detmath(_p(x), len(x), *[_p(o) for o in outs]))
    return outs


# ---- the samplers' device functions, one element per thread (include/miso_amd.h MISO_SELFTEST_*; tests/test_gpu_primitives.py) ----
SELFTEST_EXP_N, SELFTEST_LOG_N, SELFTEST_EXP_T, SELFTEST_LOG_T, SELFTEST_SQRT_POS = range(5)
(SELFTEST_K2_THRESHOLD, SELFTEST_K2_THRESHOLD_EXACT, SELFTEST_FLAT_LT, SELFTEST_FLAT_LE, SELFTEST_FLAT_GENERAL_LT,
 SELFTEST_FLAT_GENERAL_LE, SELFTEST_FLAT_FAST_LT, SELFTEST_FLAT_FAST_LE, SELFTEST_DRAW_LT, SELFTEST_DRAW_LE) = range(10)


def selftest_detmath_n(fn, x, width=1, stride=0):
    """csrc/detmath_n.hpp routine `fn` at `width` arguments per call: out[i, j] = f(x[(i + j * stride) % n])"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros((len(x), width), np.float64)
    check(lib().miso_selftest_detmath_n(int(fn), int(width), _p(x), len(x), int(stride), _p(out)))
    return out


SELFTEST_EXP_R, SELFTEST_LOG_R = range(2)
SELFTEST_ROUTE_FAST, SELFTEST_ROUTE_FULL = range(2)


def selftest_detmath_routed(fn, x, force_full=False):
    """csrc/detmath_n.hpp det_exp_r / det_log_r, the Metropolis-Hastings step's exp / log with the route chosen per
    wavefront: (values, route of each element's wavefront); element i runs on thread i (64 consecutive elements share a
    wavefront)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(len(x), np.float64)
    route = np.full(len(x), -1, np.int32)
    check(lib().miso_selftest_detmath_routed(int(fn), int(bool(force_full)), _p(x), len(x), _p(out), _p(route)))
    return out, route


def selftest_threshold(routine, c, T):
    """#{32-bit words u for which the reference's draw test holds} as threshold routine `routine` counts it; element i
    runs on thread i (64 consecutive elements share a wavefront)"""
    c = np.ascontiguousarray(c, dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    if c.shape != T.shape or c.ndim != 1:
        raise ValueError("c and T: two vectors of one length")
    out = np.zeros(len(c), np.uint64)
    check(lib().miso_selftest_threshold(int(routine), _p(c), _p(T), len(c), _p(out)))
    return out


def selftest_count_below(D, words4, T):
    """kernels_flat.inl count_below: D + (w0 < T) + (w1 < T) + (w2 < T) + (w3 < T) per element"""
    D = np.ascontiguousarray(D, dtype=np.int32)
    w = np.ascontiguousarray(words4, dtype=np.uint32).reshape(len(D), 4)
    T = np.ascontiguousarray(T, dtype=np.uint32)
    if len(T) != len(D):
        raise ValueError("D, words4 and T differ in length")
    out = np.zeros(len(D), np.int32)
    check(lib().miso_selftest_count_below(_p(D), _p(w), _p(T), len(D), _p(out)))
    return out


def selftest_pe_pick(frag, psi, fp_rep, rule_le, words):
    """One paired-end read's draw per element, as the dense read loop makes it (kernels_grp.inl pe_all_tests) and as
    pe_pick_exact does.  frag: n x K fragment indices into fp_rep, len(fp_rep) - 2 = incompatible (fp_rep there: -0.0);
    psi: n x K; rule_le: 1 = `!(rnd > c)`, 0 = `rnd < c`, then the second isoform.
    Returns (dense pick or -1 where the loop hands the read to pe_pick_exact, over[n, K - 1], pe_pick_exact's pick)."""
    frag = np.ascontiguousarray(frag, dtype=np.uint8)
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    fp = np.ascontiguousarray(fp_rep, dtype=np.float64)
    rule = np.ascontiguousarray(rule_le, dtype=np.uint32)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n, K = frag.shape
    if psi.shape != (n, K) or len(rule) != n or len(words) != n:
        raise ValueError("frag, psi: n x K; rule_le, words: n")
    out = np.zeros((n, K + 1), np.int32)
    check(lib().miso_selftest_pe_pick(K, _p(frag), _p(psi), _p(fp), len(fp), _p(rule), _p(words), n, _p(out)))
    return out[:, 0].copy(), out[:, 1:K].copy(), out[:, K].copy()


def selftest_binomial(G, n, p, count, seed=1, event_id=0):
    """`count` draws of Binomial(n, p) by kernels_k2.inl binomial_coop<G> (chain 0, iterations 0 .. count - 1)"""
    out = np.zeros(count, np.int32)
    check(lib().miso_selftest_binomial(int(G), C.c_uint64(seed), C.c_uint32(event_id), C.c_int32(n), C.c_double(p),
                                       int(count), _p(out)))
    return out


SELFTEST_LAW_INFO = ("regime", "enumerated", "total", "restarts", "out_of_range", "not_monotone", "segment_checked",
                     "segment_bad_near", "segment_bad_far")
SELFTEST_LAW_INVERSION, SELFTEST_LAW_BTRS = range(2)


def selftest_binomial_law(n, p, stride):
    """The law of include/miso_binomial.h's draws by enumeration of their 32-bit words on the device (include/miso_amd.h
    miso_selftest_binomial_law): (hist[n + 1] uint64 in terms of r = min(p, 1 - p), info as a dict of ints, kernel ms)"""
    hist = np.zeros(int(n) + 1, np.uint64)
    info = np.zeros(len(SELFTEST_LAW_INFO), np.uint64)
    ms = C.c_float(0.0)
    check(lib().miso_selftest_binomial_law(C.c_int32(n), C.c_double(p), C.c_uint32(stride), _p(hist), _p(info), C.byref(ms)))
    return hist, {k: int(v) for k, v in zip(SELFTEST_LAW_INFO, info)}, float(ms.value)


def selftest_exact(stats7, probs):
    """csrc/kernels_exact.hip, the posterior stage alone: stats7[i] = (n10, n01, n, e0, e1, h0, h1) -> (out8 [n, 8] = mean of x,
    mean of 1 - x, window low / high, normalising sum, mode, grid step, log density at the mode; icdf [n, len(probs), 2] =
    (x, 1 - x) at the inverse CDF of every probability) -- include/miso_amd.h miso_selftest_exact"""
    st = np.ascontiguousarray(stats7, dtype=np.float64).reshape(-1, 7)
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out8 = np.zeros((len(st), 8))
    icdf = np.zeros((len(st), len(pr), 2))
    check(lib().miso_selftest_exact(_p(st), len(st), _p(pr), len(pr), _p(out8), _p(icdf)))
    return out8, icdf


def selftest_exact_paired(stats6, pairs, probs):
    """csrc/kernels_exact_paired.hip, the posterior stage alone: stats6[i] = (n10, n01, A0, A1, h0, h1), pairs[i] = the
    element's drawing pairs [(m0, m1), ...] -> (out8 [n, 8] = mean of x, mean of 1 - x, window low / high, normalising sum,
    gref, grid step, log of the normalising sum + gref; icdf [n, len(probs), 2]) -- include/miso_amd.h miso_selftest_exact_paired"""
    st = np.ascontiguousarray(stats6, dtype=np.float64).reshape(-1, 6)
    if len(pairs) != len(st):
        raise ValueError("one list of pairs per element")
    rows = [np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 2) for q in pairs]
    offs = np.zeros(len(st) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    m = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 2)))
    if len(m) == 0:
        m = np.zeros((1, 2))           # (a valid pointer; no element reads it)
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out8 = np.zeros((len(st), 8))
    icdf = np.zeros((len(st), len(pr), 2))
    check(lib().miso_selftest_exact_paired(_p(st), _p(m), _p(offs), len(st), _p(pr), len(pr), _p(out8), _p(icdf)))
    return out8, icdf


def _pair_lists(stats6, pairs):
    """(stats6 [n, 6], m [*, 2], offs [n + 1]) of miso_selftest_exact_paired's layout"""
    st = np.ascontiguousarray(stats6, dtype=np.float64).reshape(-1, 6)
    if len(pairs) != len(st):
        raise ValueError("one list of pairs per element")
    rows = [np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 2) for q in pairs]
    offs = np.zeros(len(st) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    m = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 2)))
    if len(m) == 0:
        m = np.zeros((1, 2))           # (a valid pointer; no element reads it)
    return st, m, offs


def selftest_exact_paired_compare(stats6_1, pairs_1, stats6_2, pairs_2, z=()):
    """csrc/kernels_exact_paired_compare.hip on caller-given elements: stats6_s[j] = (n10, n01, A0, A1, h0, h1) and
    pairs_s[j] = [(m0, m1), ...] of pair j in sample s -> out [n, 5 + len(z)] as selftest_exact_compare's --
    include/miso_amd.h miso_selftest_exact_paired_compare"""
    s1, m1, o1 = _pair_lists(stats6_1, pairs_1)
    s2, m2, o2 = _pair_lists(stats6_2, pairs_2)
    if len(s1) != len(s2):
        raise ValueError("stats6_1, stats6_2: one row per pair each")
    zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    out = np.zeros((len(s1), 5 + len(zz)))
    check(lib().miso_selftest_exact_paired_compare(_p(s1), _p(m1), _p(o1), _p(s2), _p(m2), _p(o2), C.c_int(len(s1)),
                                                   _p(zz), C.c_int(len(zz)), _p(out)))
    return out


def selftest_exact_compare(stats7_1, stats7_2, z=()):
    """csrc/kernels_exact_compare.hip on caller-given statistics: stats7_i[j] = (n10, n01, n, e0, e1, h0, h1) of pair j in
    sample i -> out [n, 5 + len(z)] = mean1, mean2, log density of psi_1 - psi_2 at 0, Bayes factor (capped), log10 Bayes
    factor, P(psi_1 - psi_2 <= z) -- include/miso_amd.h miso_selftest_exact_compare"""
    s1 = np.ascontiguousarray(stats7_1, dtype=np.float64).reshape(-1, 7)
    s2 = np.ascontiguousarray(stats7_2, dtype=np.float64).reshape(-1, 7)
    if len(s1) != len(s2):
        raise ValueError("stats7_1, stats7_2: one row per pair each")
    zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    out = np.zeros((len(s1), 5 + len(zz)))
    check(lib().miso_selftest_exact_compare(_p(s1), _p(s2), C.c_int(len(s1)), _p(zz), C.c_int(len(zz)), _p(out)))
    return out


def selftest_exact_delta_quantiles(stats7_1, stats7_2, probs=(0.5, 0.025, 0.975)):
    """csrc/kernels_exact_delta.hip on caller-given statistics: the pairs as selftest_exact_compare's -> out [n, len(probs) + 1]
    = the quantiles of psi_1 - psi_2 at probs, then P(psi_1 - psi_2 <= 0) -- include/miso_amd.h
    miso_selftest_exact_delta_quantiles"""
    s1 = np.ascontiguousarray(stats7_1, dtype=np.float64).reshape(-1, 7)
    s2 = np.ascontiguousarray(stats7_2, dtype=np.float64).reshape(-1, 7)
    if len(s1) != len(s2):
        raise ValueError("stats7_1, stats7_2: one row per pair each")
    pp = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out = np.zeros((len(s1), len(pp) + 1))
    check(lib().miso_selftest_exact_delta_quantiles(_p(s1), _p(s2), C.c_int(len(s1)), _p(pp), C.c_int(len(pp)), _p(out)))
    return out


def selftest_exact_paired_delta_quantiles(stats6_1, pairs_1, stats6_2, pairs_2, probs=(0.5, 0.025, 0.975)):
    """csrc/kernels_exact_paired_delta.hip on caller-given elements: the pairs as selftest_exact_paired_compare's -> out
    [n, len(probs) + 1] as selftest_exact_delta_quantiles' -- include/miso_amd.h miso_selftest_exact_paired_delta_quantiles"""
    s1, m1, o1 = _pair_lists(stats6_1, pairs_1)
    s2, m2, o2 = _pair_lists(stats6_2, pairs_2)
    if len(s1) != len(s2):
        raise ValueError("stats6_1, stats6_2: one row per pair each")
    pp = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out = np.zeros((len(s1), len(pp) + 1))
    check(lib().miso_selftest_exact_paired_delta_quantiles(_p(s1), _p(m1), _p(o1), _p(s2), _p(m2), _p(o2), C.c_int(len(s1)),
                                                          _p(pp), C.c_int(len(pp)), _p(out)))
    return out


def selftest_text_digits(x):
    """csrc/text_digits.hpp text_digits per element: the digits of "%.4f" % x[i] as a signed integer (x 10^4, ties to even)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("x: one vector")
    out = np.zeros(len(x), np.int64)
    check(lib().miso_selftest_text_digits(_p(x), len(x), _p(out)))
    return out


def selftest_k2_flag(m, k, start):
    """csrc/k2_flag.hpp on the device, one lane per element: trips start[i] .. start[i + 1] - 1 of (running minimum m, stride
    position k) noted in order; returns (code, pos): 0 none / 1 exactly one flagged trip, at pos / 2 more than one"""
    m = np.ascontiguousarray(m, dtype=np.uint32)
    k = np.ascontiguousarray(k, dtype=np.uint32)
    start = np.ascontiguousarray(start, dtype=np.int32)
    if m.shape != k.shape or m.ndim != 1 or start.ndim != 1 or len(start) < 1 or start[0] != 0 or start[-1] != len(m):
        raise ValueError("m, k: two vectors of one length; start: offsets from 0 to len(m)")
    n = len(start) - 1
    code, pos = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    check(lib().miso_selftest_k2_flag(_p(m), _p(k), _p(start), n, _p(code), _p(pos)))
    return code, pos


def selftest_k2_count(th, start, u, inv, masked):
    """csrc/k2_count.hpp's assembly statements on the device, one lane per element: words start[i] .. start[i + 1] - 1 of u
    (an even number), two per statement, against high-half threshold th[i]; masked[i] != 0: the tail's form, inv = the halves
    that are not reads; 0: the steady trips' form (inv must be 0).  Returns (acc, o): the packed sums and the flag word"""
    th = np.ascontiguousarray(th, dtype=np.uint32)
    u = np.ascontiguousarray(u, dtype=np.uint32)
    inv = np.ascontiguousarray(inv, dtype=np.uint32)
    masked = np.ascontiguousarray(masked, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int32)
    if (u.shape != inv.shape or u.ndim != 1 or start.ndim != 1 or len(start) < 1 or start[0] != 0 or start[-1] != len(u)
            or th.shape != (len(start) - 1,) or masked.shape != th.shape):
        raise ValueError("u, inv: two vectors of one length; start: offsets from 0 to len(u); th, masked: one per sequence")
    n = len(start) - 1
    acc, o = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    check(lib().miso_selftest_k2_count(_p(th), _p(start), _p(u), _p(inv), _p(masked), n, _p(acc), _p(o)))
    return acc, o


def selftest_k2_finish(seed, event_id, chain, iteration, n_draw, t, settle_all=False):
    """csrc/kernels_k2.inl k2_finish_lane on the device, one single-lane chain per element: the number of the chain's n_draw[i]
    drawing reads at iteration[i] whose uniform is below the caller's threshold t[i] (0 .. 2^32), through the read loop's sum
    and flag, the settle path and the finishing expression -- include/miso_amd.h miso_selftest_k2_finish"""
    event_id = np.ascontiguousarray(event_id, dtype=np.uint32)
    chain = np.ascontiguousarray(chain, dtype=np.uint32)
    iteration = np.ascontiguousarray(iteration, dtype=np.uint32)
    n_draw = np.ascontiguousarray(n_draw, dtype=np.int32)
    t = np.ascontiguousarray(t, dtype=np.uint64)
    n = len(t)
    if any(a.shape != (n,) for a in (event_id, chain, iteration, n_draw)):
        raise ValueError("event_id, chain, iteration, n_draw, t: one entry per element")
    out = np.zeros(n, np.int32)
    check(lib().miso_selftest_k2_finish(C.c_uint64(seed), _p(event_id), _p(chain), _p(iteration), _p(n_draw), _p(t),
                                        C.c_int(int(bool(settle_all))), C.c_int(n), _p(out)))
    return out


def selftest_convergent_mean(samples, chains):
    """samples: S x K (row i from chain i % chains) -> True if stop=CONVERGENT_MEAN would stop (miso.c:556-636)"""
    a = np.ascontiguousarray(samples, dtype=np.float64)
    stop = C.c_int(-1)
    check(lib().miso_selftest_convergent_mean(_p(a), a.shape[1], int(chains), a.shape[0], C.byref(stop)))
    return bool(stop.value)


def selftest_knobs():
    """{name: value text} of the MISO_* tuning knobs that are set, as the planner would read them now (csrc/knobs.hpp)"""
    need = lib().miso_selftest_knobs(None, 0)
    if need < 0:
        raise MemoryError("miso_selftest_knobs")
    buf = C.create_string_buffer(need)
    lib().miso_selftest_knobs(buf, need)
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def selftest_philox(ctr_key6):
    a = np.ascontiguousarray(ctr_key6, dtype=np.uint32).reshape(-1, 6)
    out = np.zeros((len(a), 4), np.uint32)
    check(lib().miso_selftest_philox(_p(a), len(a), _p(out)))
    return out


# ---- the fragment length distribution of a paired-end file (include/miso_alnio.h miso_insert_len) ----
MISO_INSERT_TAG_MASK, MISO_INSERT_TAG_NONE, MISO_INSERT_TAG_MULTI = 0x1FFFFFFF, 0x1FFFFFFF, 0x1FFFFFFE
MISO_INSERT_ONE_M, MISO_INSERT_FILTER_OK = 1 << 29, 1 << 30


class InsertStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("kept", "skipped", "unpaired", "same_strand", "nonpositive", "tagged",
                                          "chunks")]
                + [(n, C.c_double) for n in ("records_ms", "grouping_ms", "pairs_ms")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _intervals(seqids, starts, ends):
    n = len(seqids)
    # one C string per distinct name and an array of their addresses (an annotation has 10^5 - 10^6 intervals on a few
    # dozen names: setting a c_char_p array entry by entry costs more than the device pass it feeds)
    held = {s: C.create_string_buffer(s.encode() if isinstance(s, str) else s) for s in set(seqids)}
    addr = {s: C.addressof(b) for s, b in held.items()}
    ptrs = np.zeros(max(n, 1), np.uint64)
    ptrs[:n] = [addr[s] for s in seqids]
    names = (C.c_char_p * max(n, 1)).from_buffer(ptrs)      # shares ptrs' memory and keeps it alive
    names.held = held
    st = np.ascontiguousarray(starts, dtype=np.int64)
    en = np.ascontiguousarray(ends, dtype=np.int64)
    if len(st) != n or len(en) != n:
        raise ValueError("seqids, starts and ends differ in length")
    return n, names, st, en


_INSERT_ARGS = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]


def insert_tag_records(alnfile, seqids, starts, ends, device=0, filter_reads=True, chunk_records=0):
    """The record pass alone: one MISO_INSERT_* code per record of an open alignment file (sam_utils.Samfile);
    intervals in GFF coordinates (1-based, inclusive)."""
    n, names, st, en = _intervals(seqids, starts, ends)
    codes = np.zeros(max(len(alnfile), 1), np.int32)
    L = lib()
    L.miso_insert_tag_records.argtypes = _INSERT_ARGS + [C.c_void_p]
    check(L.miso_insert_tag_records(alnfile._h, int(device), int(bool(filter_reads)), n, names, _p(st), _p(en),
                                    int(chunk_records), _p(codes)))
    return codes[:len(alnfile)]


def insert_len(alnfile, seqids, starts, ends, device=0, filter_reads=True, chunk_records=0):
    """Tag, pair and measure on the device (miso_insert_len).  Returns (interval index[], insert[], stats dict): the kept
    pairs ordered by interval index, then by the left mate's place in the file."""
    n, names, st, en = _intervals(seqids, starts, ends)
    cap = len(alnfile) // 2          # no file holds more pairs: one call, no second pass for the size
    iv = np.zeros(max(cap, 1), np.int32)
    ins = np.zeros(max(cap, 1), np.int32)
    kept = C.c_int64(0)
    stats = InsertStats()
    L = lib()
    L.miso_insert_len.argtypes = _INSERT_ARGS + [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                                 C.POINTER(InsertStats)]
    check(L.miso_insert_len(alnfile._h, int(device), int(bool(filter_reads)), n, names, _p(st), _p(en),
                            int(chunk_records), _p(iv), _p(ins), cap, C.byref(kept), C.byref(stats)))
    k = kept.value
    return iv[:k].copy(), ins[:k].copy(), stats.as_dict()


# ---- per-interval read coverage (include/miso_alnio.h miso_region_counts) ----
class RegionStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("kept", "chunks")]
                + [(n, C.c_double) for n in ("records_ms", "sort_ms", "rank_ms", "total_ms")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def region_counts(alnfile, seqids, starts, ends, device=0, chunk_records=0):
    """Kept records (mapped, span held whole by some interval) overlapping each interval of an open alignment file
    (sam_utils.Samfile), intervals in GFF coordinates (1-based, inclusive), seqids spelled as the file spells them.
    Returns (int64 counts per interval, stats dict)."""
    n, names, st, en = _intervals(seqids, starts, ends)
    counts = np.zeros(max(n, 1), np.int64)
    stats = RegionStats()
    L = lib()
    L.miso_region_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.POINTER(RegionStats)]
    check(L.miso_region_counts(alnfile._h, int(device), n, names, _p(st), _p(en), int(chunk_records), _p(counts),
                               C.byref(stats)))
    return counts[:n].copy(), stats.as_dict()


# ---- fetch counts of many intervals (include/miso_alnio.h miso_fetch_counts) ----
def fetch_counts(alnfile, seqids, starts, ends, device=0, chunk_records=0):
    """len(bamfile.fetch(seqid, start, end)) for every interval of an open alignment file (sam_utils.Samfile) in one
    device pass: the records on the reference named seqid with pos < end and bam_endpos > start, the numbers used as
    given, seqids spelled as the file spells them.  Returns (int64 counts per interval, stats dict)."""
    n, names, st, en = _intervals(seqids, starts, ends)
    counts = np.zeros(max(n, 1), np.int64)
    stats = RegionStats()
    L = lib()
    L.miso_fetch_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.POINTER(RegionStats)]
    check(L.miso_fetch_counts(alnfile._h, int(device), n, names, _p(st), _p(en), int(chunk_records), _p(counts),
                              C.byref(stats)))
    return counts[:n].copy(), stats.as_dict()


# ---- per-base read density and junction counts (include/miso_alnio.h miso_region_densities) ----
class DensityStats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("fetched", "skipped_multi_n", "skipped_no_cigar", "with_indel", "qlen_classes",
                                          "chunks", "groups", "junction_retries")]
                + [(n, C.c_double) for n in ("tables_ms", "mark_ms", "records_ms", "scan_ms", "junction_ms", "copy_ms",
                                             "total_ms")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def region_densities(alnfile, seqids, starts, ends, device=0, chunk_records=0, accum_bytes=0):
    """Read density and junctions of every region (seqid, tx_start, tx_end), GFF numbers, of an open alignment file
    (sam_utils.Samfile) in one device pass; seqids spelled as the file spells them.  Returns (depth, wiggle, junctions,
    stats): per region an int32 array and a float64 array of tx_end - tx_start + 1 entries (empty when
    tx_start > tx_end) and a list of (leftss, rightss, count) sorted by the splice sites; stats as a dict."""
    n, names, st, en = _intervals(seqids, starts, ends)
    lens = np.maximum(en - st + 1, 0) if n else np.zeros(0, np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    total = int(off[-1])
    depth = np.zeros(max(total, 1), np.int32)
    wiggle = np.zeros(max(total, 1), np.float64)
    stats = DensityStats()
    found = C.c_int64(0)
    L = lib()
    L.miso_region_densities.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
                                        + [C.c_int64, C.POINTER(C.c_int64), C.POINTER(DensityStats)])
    cap = 1 << 16
    while True:
        jr, jl = np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        jrt, jc = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        check(L.miso_region_densities(alnfile._h, int(device), n, names, _p(st), _p(en), int(chunk_records),
                                      int(accum_bytes), _p(depth), _p(wiggle), total, _p(jr), _p(jl), _p(jrt), _p(jc),
                                      cap, C.byref(found), C.byref(stats)))
        if found.value <= cap:
            break
        cap = found.value            # the list did not fit: once more, with room for all of it
    junctions = [[] for _ in range(n)]
    for k in range(found.value):
        junctions[jr[k]].append((int(jl[k]), int(jrt[k]), int(jc[k])))
    return ([depth[off[i]:off[i + 1]].copy() for i in range(n)], [wiggle[off[i]:off[i + 1]].copy() for i in range(n)],
            junctions, stats.as_dict())
