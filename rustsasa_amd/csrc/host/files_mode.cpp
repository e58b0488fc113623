// Host API, part 5 of 5: the four level processors of the reference's src/options.rs - one GPU batch for a set of
// prepared structures, results per level - and directory mode (SASAOptions::process_files).
#include "host_internal.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <malloc.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <type_traits>

namespace rustsasa {
namespace detail {

namespace {

// process_atoms of each level (options.rs:142-149, 195-232, 292-315, 370-410).  `atom` and
// `seg` are this structure's slices of the batch results; `global` is the sequential f32 sum
// over all its atoms (used by ProteinLevel only).
template <typename Level>
typename Level::Output finish(const Structure &pdb, const float *atom, size_t n_atoms,
                              const float *seg, float global);

template <>
std::vector<float> finish<AtomLevel>(const Structure &, const float *atom, size_t n, const float *, float)
{
    return std::vector<float>(atom, atom + n);
}

template <>
std::vector<ResidueResult> finish<ResidueLevel>(const Structure &pdb, const float *, size_t,
                                                const float *seg, float)
{
    std::vector<ResidueResult> out;
    size_t k = 0;
    for (const Chain &chain : pdb.chains)
        for (const Residue &res : chain.residues) {
            std::string name;
            res.name(&name);
            out.push_back(ResidueResult{res.serial_number, res.insertion_code, seg[k++], name,
                                        is_polar_residue(name), chain.id});
        }
    return out;
}

// ChainLevel keeps the serialize_chain_id key: chains whose ids serialise to the same number
// share the map entry of the LAST of them (parent_to_atoms.insert overwrites, options.rs:361).
template <>
std::vector<ChainResult> finish<ChainLevel>(const Structure &pdb, const float *, size_t,
                                            const float *seg, float)
{
    std::map<std::int64_t, size_t> key_to_chain;
    for (size_t ci = 0; ci < pdb.chains.size(); ci++)
        key_to_chain[serialize_chain_id(pdb.chains[ci].id)] = ci;
    std::vector<ChainResult> out;
    for (const Chain &chain : pdb.chains)
        out.push_back(ChainResult{chain.id, seg[key_to_chain[serialize_chain_id(chain.id)]]});
    return out;
}

template <>
ProteinResult finish<ProteinLevel>(const Structure &pdb, const float *, size_t, const float *seg,
                                   float global)
{
    float polar = 0.f, non_polar = 0.f;  // options.rs:376-402
    size_t k = 0;
    for (const Chain &chain : pdb.chains)
        for (const Residue &res : chain.residues) {
            std::string name;
            res.name(&name);
            if (is_polar_residue(name)) polar += seg[k]; else non_polar += seg[k];
            k++;
        }
    return ProteinResult{global, polar, non_polar};  // global_total = simd_sum(atom_sasa), :404
}

std::string engine_message(const OptionValues &o, int rc)
{
    std::string m = std::string("rustsasa_amd engine: ") + rsasa_status_string(rc);
    if (o.context) m += std::string(": ") + rsasa_context_last_error(o.context);
    return m;
}

// CPUs this process can really use: the hardware threads, capped by its cgroup's CPU quota (cgroup v2 cpu.max).  A
// container limited to 16 CPUs on a 256-thread host gets 16 threads' worth of time however many threads it starts;
// a pool sized by hardware_concurrency() there spends its time being throttled (the measurement boxes are such
// containers: that is why 64 parse threads were slower than 32 there).
unsigned effective_cpus()
{
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long long period = 0;
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
            const long long quota = std::atoll(q);
            if (quota > 0) n = std::min(n, (unsigned)std::max(1ll, (quota + period / 2) / period));
        }
        std::fclose(f);
    }
    return n;
}

// Static-chunked parallel loop over [0, n) on up to `threads` std::threads (host glue only).
template <typename F>
void parallel_for(size_t n, unsigned threads, F body)
{
    const unsigned nt = (unsigned)std::min<size_t>(std::max(1u, threads), n);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++) body(i);
        return;
    }
    std::atomic<size_t> next{0};
    auto worker = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < n;) body(i);
    };
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < nt; k++) pool.emplace_back(worker);
    worker();
    for (auto &th : pool) th.join();
}

// Runs the GPU once for a set of prepared structures (those without a build error) and turns
// the results into per-structure level outputs.  Build errors stay with their structure and do
// not disturb the others (reference src/main.rs:446-454).
// `out_paths` (process_files with OptionValues::output_dir): the file a structure's result goes to as JSON, written by
// the thread that builds the result (bytes written are added to *bytes_written).
template <typename Level>
void run_batch(const OptionValues &o, const std::vector<const Structure *> &pdbs,
               std::vector<Prepared> &prep, std::vector<Result<typename Level::Output>> &out,
               unsigned host_threads = 1, const std::string *out_paths = nullptr, std::atomic<uint64_t> *bytes_written = nullptr)
{
    const size_t n_files = pdbs.size();
    out.assign(n_files, Result<typename Level::Output>());
    std::vector<uint32_t> s_off{0u}, seg_off{0u};
    std::vector<size_t> members;
    size_t n_total = 0;
    for (size_t f = 0; f < n_files; f++) {
        if (prep[f].err.error != SASACalcError::Ok) {
            out[f].error = prep[f].err.error;
            out[f].message = prep[f].err.message;
            continue;
        }
        members.push_back(f);
        for (uint32_t e : prep[f].seg_end) seg_off.push_back((uint32_t)n_total + e);
        n_total += prep[f].atoms.size();
        s_off.push_back((uint32_t)n_total);
    }
    if (members.empty()) return;
    const bool trace = rsasa::tuning_env("RSASA_FILES_TRACE") != nullptr;
    const auto tr0 = std::chrono::steady_clock::now();
    std::vector<float> x(n_total), y(n_total), z(n_total), rad(n_total), atom(n_total, 0.f);
    std::vector<std::uint64_t> id(n_total);
    parallel_for(members.size(), host_threads, [&](size_t m) {
        size_t i = s_off[m];
        for (const rsasa_atom_t &a : prep[members[m]].atoms) {
            x[i] = a.position[0]; y[i] = a.position[1]; z[i] = a.position[2];
            rad[i] = a.radius; id[i] = a.id;
            i++;
        }
    });
    const size_t n_seg = seg_off.size() - 1;
    std::vector<float> seg(n_seg, 0.f), global(members.size(), 0.f);
    int rc = RSASA_OK;
    const auto tr1 = std::chrono::steady_clock::now();
    if (n_total) {  // calculate_sasa_internal on an empty slice returns an empty Vec
        rc = rsasa_calculate_sasa_batch(o.context, x.data(), y.data(), z.data(), rad.data(), id.data(),
                                        s_off.data(), members.size(), o.probe_radius, o.n_points,
                                        atom.data(), n_seg ? seg_off.data() : nullptr, n_seg,
                                        n_seg ? seg.data() : nullptr);
        if (rc == RSASA_OK && std::is_same<Level, ProteinLevel>::value)
            rc = rsasa_segment_sums(o.context, atom.data(), n_total, s_off.data(), members.size(),
                                    global.data());
    }
    const auto tr2 = std::chrono::steady_clock::now();
    std::vector<size_t> seg_pos(members.size() + 1, 0);
    for (size_t m = 0; m < members.size(); m++) seg_pos[m + 1] = seg_pos[m] + prep[members[m]].seg_end.size();
    const std::string engine_err = rc != RSASA_OK ? engine_message(o, rc) : std::string();
    parallel_for(members.size(), host_threads, [&](size_t m) {
        const size_t f = members[m];
        if (rc != RSASA_OK) {
            out[f].error = SASACalcError::Engine;
            out[f].message = engine_err;
            return;
        }
        out[f].value = finish<Level>(*pdbs[f], atom.data() + s_off[m], prep[f].atoms.size(),
                                     seg.data() + seg_pos[m], global[m]);
        if (out_paths) {  // reference src/main.rs:208-211: sasa_result_to_json + fs::write, per file
            const std::string text = sasa_result_to_json(out[f].value);
            std::string err;
            if (!write_whole_file(out_paths[f], text, &err)) {
                out[f].error = SASACalcError::Engine;
                out[f].message = err;
            } else if (bytes_written) {
                bytes_written->fetch_add(text.size(), std::memory_order_relaxed);
            }
        }
    });
    if (trace) {
        const auto tr3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "run_batch: %zu files %zu atoms: pack %.2f ms, engine %.2f ms, results %.2f ms\n", n_files, n_total,
                     ms(tr0, tr1), ms(tr1, tr2), ms(tr2, tr3));
    }
}

}  // namespace

Result<std::vector<float>> run_hot_path(const OptionValues &o, const std::vector<rsasa_atom_t> &atoms)
{
    Result<std::vector<float>> out;
    out.value.assign(atoms.size(), 0.f);
    if (atoms.empty()) return out;
    const int rc = rsasa_calculate_sasa_internal(o.context, atoms.data(), atoms.size(),
                                                 o.probe_radius, o.n_points, o.threads,
                                                 out.value.data());
    if (rc != RSASA_OK) {
        out.error = SASACalcError::Engine;
        out.message = engine_message(o, rc);
    }
    return out;
}

template <typename Level>
std::vector<Result<typename Level::Output>> process_many(const std::vector<const Structure *> &pdbs,
                                                         const OptionValues &o)
{
    std::vector<Prepared> prep(pdbs.size());
    for (size_t f = 0; f < pdbs.size(); f++) prep[f] = prepare(*pdbs[f], o, level_index<Level>::value);
    std::vector<Result<typename Level::Output>> out;
    run_batch<Level>(o, pdbs, prep, out);
    return out;
}

namespace {

// A queue that holds at most `capacity` items: push waits for room, pop for an item.  pop returns an empty T only when
// the queue is closed and drained.
template <typename T>
class BoundedQueue {
    std::mutex mu;
    std::condition_variable cv_room, cv_item;
    std::deque<T> items;
    bool closed = false;
    const size_t capacity;

  public:
    explicit BoundedQueue(size_t capacity_) : capacity(capacity_) {}
    void push(T item)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_room.wait(lk, [&] { return items.size() < capacity; });
        items.push_back(std::move(item));
        lk.unlock();
        cv_item.notify_one();
    }
    T pop()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_item.wait(lk, [&] { return closed || !items.empty(); });
        if (items.empty()) return T();
        T item = std::move(items.front());
        items.pop_front();
        lk.unlock();
        cv_room.notify_one();
        return item;
    }
    void close()
    {
        std::unique_lock<std::mutex> lk(mu);
        closed = true;
        lk.unlock();
        cv_item.notify_all();
    }
};

// process_files' cached second context per device (see borrow_companion)
struct Companion {
    rsasa_context_t *ctx = nullptr;
    bool busy = false;
};
std::mutex &companions_mutex()
{
    static std::mutex *m = new std::mutex();  // (never destroyed: the atexit handler below may run after other statics)
    return *m;
}
std::map<int, Companion> &companions_map()
{
    static std::map<int, Companion> *m = new std::map<int, Companion>();
    return *m;
}

}  // namespace

void release_cached_contexts_impl()
{
    std::lock_guard<std::mutex> lk(companions_mutex());
    auto &m = companions_map();
    for (auto it = m.begin(); it != m.end();) {
        if (it->second.busy) { ++it; continue; }  // (a process_files call is running with it)
        if (it->second.ctx) rsasa_context_destroy(it->second.ctx);
        it = m.erase(it);
    }
}

namespace {

// A second context on the device of `first`, for the duration of a process_files call (calls on one context are
// serialised).  The companion context is kept for the life of the process, one per device (a context is a GPU workspace
// and a few threads: creating one per call cost more than the call's second chunk); a call that finds it taken creates
// its own.  It runs with the caller's context's settings: the pulp lane count decides which points take the remainder
// rule, and chunks go to whichever worker is free (the caller clones the settings).  `ctx` is null when there is none.
// The cached companions are released when the process ends normally, BEFORE the HIP runtime's own static teardown
// (atexit handlers registered later run earlier; this one is registered after the first context exists, i.e. after
// the runtime started up); rustsasa::release_cached_contexts() does the same on request - a long-lived host program
// that is done with directory mode gets its HBM workspaces, pinned staging and coding threads back.
struct Borrowed {
    rsasa_context_t *ctx = nullptr;
    int device = -1;
    bool cached = false;
    Borrowed() = default;
    Borrowed(Borrowed &&other) noexcept : ctx(other.ctx), device(other.device), cached(other.cached) { other.ctx = nullptr; other.cached = false; }
    ~Borrowed()
    {
        if (cached) {
            std::lock_guard<std::mutex> lk(companions_mutex());
            companions_map()[device].busy = false;
        } else if (ctx) {
            rsasa_context_destroy(ctx);
        }
    }
};

Borrowed borrow_companion(rsasa_context_t *first)
{
    static const bool registered = (std::atexit([] { release_cached_contexts_impl(); }), true);
    (void)registered;
    Borrowed second;
    if (rsasa_context_get_device(first, &second.device) != RSASA_OK) second.device = 0;
    {
        std::lock_guard<std::mutex> lk(companions_mutex());
        Companion &c = companions_map()[second.device];
        if (!c.busy) {
            if (!c.ctx && rsasa_context_create(second.device, &c.ctx) != RSASA_OK) c.ctx = nullptr;
            if (c.ctx) {
                c.busy = true;
                second.ctx = c.ctx;
                second.cached = true;
            }
        }
    }
    if (!second.ctx && rsasa_context_create(second.device, &second.ctx) != RSASA_OK) second.ctx = nullptr;
    return second;
}

// OptionValues::output_dir: every file's result also goes to <output_dir>/<file stem>.json (reference
// src/main.rs:395-403: file_stem + the format's extension)
std::vector<std::string> output_paths(const std::vector<std::string> &paths, const std::string &output_dir)
{
    std::vector<std::string> out(output_dir.empty() ? 0 : paths.size());
    for (size_t i = 0; i < out.size(); i++) {
        const size_t slash = paths[i].find_last_of('/');
        std::string stem = paths[i].substr(slash == std::string::npos ? 0 : slash + 1);
        const size_t dot = stem.find_last_of('.');
        if (dot != std::string::npos && dot > 0) stem.resize(dot);
        out[i] = output_dir + "/" + stem + ".json";
    }
    return out;
}

// Directory mode allocates and frees a few thousand small blocks per file on every thread.  With
// glibc's defaults the heaps are trimmed and regrown all the time (brk / mprotect / page faults
// under the process-wide mapping lock) and parsing stops scaling at a dozen threads; keeping freed
// memory and growing the heaps in large steps makes the whole mode twice as fast (measured: 5.2 k
// -> 10-12 k files/s).  Process-wide, once; RSASA_KEEP_MALLOC_DEFAULTS=1 leaves malloc alone.
void tune_malloc_once()
{
    static std::once_flag malloc_once;
    std::call_once(malloc_once, [] {
        if (rsasa::tuning_env("RSASA_KEEP_MALLOC_DEFAULTS")) return;
        mallopt(M_TRIM_THRESHOLD, 1 << 30);
        mallopt(M_TOP_PAD, 256 << 20);
        mallopt(M_MMAP_THRESHOLD, 32 << 20);
    });
}

}  // namespace

// Directory mode at library level (reference src/main.rs:342-480 without the CLI): files are
// parsed and filtered on `host_threads` threads, then each chunk of `files_per_batch` structures
// is ONE GPU batch.
template <typename Level>
std::vector<Result<typename Level::Output>> process_files(const std::vector<std::string> &paths,
                                                          const OptionValues &o, unsigned host_threads,
                                                          size_t files_per_batch, FilesTimings *timings)
{
    using Clock = std::chrono::steady_clock;
    tune_malloc_once();
    std::vector<Result<typename Level::Output>> all(paths.size());
    const std::vector<std::string> out_paths = output_paths(paths, o.output_dir);  // written beside the GPU workers' result building
    std::atomic<uint64_t> bytes_written{0};
    // parsing is allocation heavy and stops scaling early (measured: 32 threads are the optimum on a
    // 256-thread host, 64 are slower), so the default is capped
    // (under a CPU quota twice the quota's threads: the parse threads also wait - for the page cache, for the chunk
    // barrier; measured with cpu.max = 16 CPUs: 16 threads 26 k files/s, 24: 33 k, 32: 37 k)
    if (host_threads == 0) host_threads = std::min(32u, 2u * effective_cpus());
    // (chunks of 512 files and two GPU workers: 16.4 k files/s on the 4 363-file set against 13.3 k with 256 and one
    // shared context - fewer per-chunk joins of the parse pool, and one chunk's upload beside the other's kernels)
    if (files_per_batch == 0) files_per_batch = 512;
    const bool fast_reader = rsasa::tuning_env("RSASA_NO_FAST_READER") == nullptr;
    // one worker per given context; with a single context a second, private one on the same device joins it
    std::vector<rsasa_context_t *> contexts = o.contexts;
    if (contexts.empty()) contexts.push_back(o.context);
    const bool two_workers = contexts.size() == 1 && paths.size() > files_per_batch;
    const Borrowed second = two_workers ? borrow_companion(contexts[0]) : Borrowed();
    // (every setting that changes how the caller's context computes: lane count, kernel tuning; no second context:
    // two workers share the one)
    if (two_workers)
        contexts.push_back(second.ctx && rsasa_context_clone_settings(second.ctx, contexts[0]) == RSASA_OK ? second.ctx : contexts[0]);

    struct Chunk {
        size_t base = 0, n = 0;
        std::vector<Structure> pdbs;
        std::vector<Prepared> prep;
    };
    // the producer (this thread + its parse pool) stays at most one chunk per worker ahead, so memory holds a few
    // chunks of parsed structures, not the whole directory
    BoundedQueue<std::unique_ptr<Chunk>> parsed(contexts.size() + 1);
    FilesTimings t{};
    std::mutex mu_t;

    // Destroying a chunk's structures competes with the parse pool: free() takes the lock of the arena a block came
    // from - the arenas the parse threads are allocating from.  Measured on the 4 363-file set (32 parse threads, one
    // block per vector of the model): freed by 16 threads on the GPU workers' path the parse pool needed 0.17-0.25 s of
    // wall time per call, by 4 threads 0.10 s, by one 0.07 s (but then the freeing itself took 0.25 s).  Hence the
    // per-structure pools (include/rustsasa_amd.hpp) and ONE reaper with a few threads, off everybody's path.
    BoundedQueue<std::unique_ptr<Chunk>> dead(4);  // (memory stays bounded if freeing falls behind)
    const unsigned free_threads = 4;
    std::thread reaper([&] {
        while (std::unique_ptr<Chunk> c = dead.pop())
            parallel_for(c->n, free_threads, [&](size_t i) {
                Structure s = std::move(c->pdbs[i]);
                Prepared pr = std::move(c->prep[i]);
            });
    });
    auto worker = [&](rsasa_context_t *ctx) {
        OptionValues mine = o;
        mine.context = ctx;
        (void)rsasa_context_bind_thread(ctx, nullptr);  // multi-socket hosts: this worker next to its GPU's link
        {
            int w = 0;
            (void)rsasa_context_get_simd_width(ctx, &w);
            std::lock_guard<std::mutex> lk(mu_t);
            t.worker_simd_widths.push_back(w);
        }
        // the first touch of a context initialises the HIP runtime (a quarter of a second): do it
        // here, while the producer parses the first chunk
        (void)rsasa_segment_sums(ctx, nullptr, 0, nullptr, 0, nullptr);
        while (std::unique_ptr<Chunk> c = parsed.pop()) {
            const auto t1 = Clock::now();
            std::vector<const Structure *> ptrs(c->n);
            for (size_t i = 0; i < c->n; i++) ptrs[i] = &c->pdbs[i];
            std::vector<Result<typename Level::Output>> out;
            run_batch<Level>(mine, ptrs, c->prep, out, std::max(1u, host_threads / 2), out_paths.empty() ? nullptr : out_paths.data() + c->base,
                             &bytes_written);
            for (size_t i = 0; i < c->n; i++) all[c->base + i] = std::move(out[i]);
            dead.push(std::move(c));  // the parsed structures (millions of small blocks) go to the reaper thread
            const double dt = std::chrono::duration<double>(Clock::now() - t1).count();
            std::lock_guard<std::mutex> lk(mu_t);
            t.compute_seconds += dt;
        }
    };
    const auto t_begin = Clock::now();
    std::vector<std::thread> workers;
    for (rsasa_context_t *ctx : contexts) workers.emplace_back(worker, ctx);

    for (size_t base = 0; base < paths.size(); base += files_per_batch) {
        auto c = std::make_unique<Chunk>();
        c->base = base;
        c->n = std::min(files_per_batch, paths.size() - base);
        c->pdbs.resize(c->n);
        c->prep.resize(c->n);
        const auto t0 = Clock::now();
        // largest files first: the chunk's parse ends with the pool, not with one thread on a 2 MB file
        std::vector<std::pair<uint64_t, size_t>> order(c->n);
        for (size_t i = 0; i < c->n; i++) {
            struct stat st{};
            order[i] = {::stat(paths[base + i].c_str(), &st) == 0 ? (uint64_t)st.st_size : 0u, i};
        }
        std::sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
        parallel_for(c->n, host_threads, [&](size_t k) {
            const size_t i = order[k].second;
            const std::string &path = paths[base + i];
            try {
                prepare_text(read_whole_file(path), is_mmcif_path(path), o, level_index<Level>::value, fast_reader,
                             !o.read_radii_from_occupancy, c->pdbs[i], c->prep[i]);
            } catch (const std::exception &e) {  // unreadable file: report, keep going (main.rs:446-454)
                c->prep[i] = Prepared{};
                c->prep[i].err = {SASACalcError::Engine, std::string("cannot read structure: ") + e.what()};
            }
        });
        size_t atoms = 0;
        for (size_t i = 0; i < c->n; i++) atoms += c->prep[i].atoms.size();
        {
            std::lock_guard<std::mutex> lk(mu_t);
            t.parse_seconds += std::chrono::duration<double>(Clock::now() - t0).count();
            t.n_atoms += atoms;
        }
        parsed.push(std::move(c));
    }
    parsed.close();
    for (auto &th : workers) th.join();
    dead.close();
    reaper.join();
    t.total_seconds = std::chrono::duration<double>(Clock::now() - t_begin).count();
    t.n_files = paths.size();
    t.bytes_written = bytes_written.load();
    if (timings) *timings = t;
    return all;
}

#define RSASA_INSTANTIATE(L)                                                                          \
    template std::vector<Result<L::Output>> process_many<L>(const std::vector<const Structure *> &,  \
                                                            const OptionValues &);                   \
    template std::vector<Result<L::Output>> process_files<L>(const std::vector<std::string> &,       \
                                                             const OptionValues &, unsigned, size_t, \
                                                             FilesTimings *);
RSASA_INSTANTIATE(AtomLevel)
RSASA_INSTANTIATE(ResidueLevel)
RSASA_INSTANTIATE(ChainLevel)
RSASA_INSTANTIATE(ProteinLevel)
#undef RSASA_INSTANTIATE

}  // namespace detail

void release_cached_contexts() { detail::release_cached_contexts_impl(); }

template <typename Level>
Result<typename Level::Output> SASAOptions<Level>::process(const Structure &pdb) const
{
    return std::move(detail::process_many<Level>({&pdb}, o_)[0]);
}

template <typename Level>
std::vector<Result<typename Level::Output>> SASAOptions<Level>::process_files(
    const std::vector<std::string> &paths, unsigned host_threads, size_t files_per_batch,
    FilesTimings *timings) const
{
    return detail::process_files<Level>(paths, o_, host_threads, files_per_batch, timings);
}

template class SASAOptions<AtomLevel>;
template class SASAOptions<ResidueLevel>;
template class SASAOptions<ChainLevel>;
template class SASAOptions<ProteinLevel>;

}  // namespace rustsasa
