// wavefront.h -- which (pass, view) a free lane of the in-memory scheduler may take when one rank runs the passes of a pyramid level
// without a barrier between them (host/multi_device.cpp, RunLevelWavefront).  Pure bookkeeping: no device call, no thread and no
// lock in here -- the scheduler calls every member while it holds its done_m, and tests/test_wavefront_queue.py drives the same
// class through host_capi.cpp on a machine without a device.
//
// A (view, pass) task needs exactly what it reads: its own previous pass; in a geometric pass the depth maps of its sources --
// this pass's for the sources that precede it and the previous pass's for the others in the reference's order (Gauss-Seidel), the
// previous pass's for all with --jacobi; and nobody may still read the two-passes-old depth map its export overwrites (depth maps
// live in two versions by pass parity).  View 0 of pass p + 1 starts while the last views of pass p are still in their second
// halves: the chains of consecutive passes overlap.
#ifndef APD_MI355X_HOST_WAVEFRONT_H_
#define APD_MI355X_HOST_WAVEFRONT_H_

#include <utility>
#include <vector>

#ifndef APD_GS_LANES_PER_PASS
#define APD_GS_LANES_PER_PASS 2  // lanes that may work on one geometric pass in the reference's order (its second halves form a chain); 24 x 1080p passes: 1: 8.16 s, 2: 7.95, 3: 7.89, 9: 7.99 (profiles/r04/ab_gs_lanes_per_pass_tt24.txt)
#endif

class WavefrontQueue {
public:
    struct PassInfo {
        int iteration = 0;   // Pass::iteration; consecutive over the passes of a level
        bool geom_consistency = false;
    };
    enum class Next { kTask, kWait, kFinished };

    // passes: those of one level, in order.  sources[v]: the views (indices below sources.size()) that view v lists as sources;
    // source-only images are left out, they have no depth map.  Every view counts as published at the iteration before the level's
    // first: levels follow one another with a barrier.
    WavefrontQueue(std::vector<PassInfo> passes, std::vector<std::vector<int>> sources, bool gauss_seidel, int lanes_per_pass = APD_GS_LANES_PER_PASS)
        : passes_(std::move(passes)), sources_(std::move(sources)), gauss_seidel_(gauss_seidel), lanes_per_pass_(lanes_per_pass)
    {
        const int V = (int)sources_.size();
        readers_.resize(V);
        for (int v = 0; v < V; ++v) {
            for (int u : sources_[v]) {
                readers_[u].push_back(v);
            }
        }
        published_.assign(V, passes_.empty() ? -1 : passes_[0].iteration - 1);
        remaining_.assign(passes_.size(), V);
        frontier_.assign(passes_.size(), 0);
        active_.assign(passes_.size(), 0);
    }

    // The task a free lane takes.  Within a pass the views go out in order; the earliest pass that has an eligible view wins.
    // kWait: tasks are left but none is eligible before a running one publishes or finishes; kFinished: every task is handed out.
    Next Take(int &pi_out, int &v_out)
    {
        const int V = (int)sources_.size();
        bool any_left = false;
        for (int pi = 0; pi < (int)passes_.size(); ++pi) {
            if (frontier_[pi] >= V) {
                continue;
            }
            any_left = true;
            if (Eligible(pi, frontier_[pi])) {
                pi_out = pi;
                v_out = frontier_[pi]++;
                ++active_[pi];
                return Next::kTask;
            }
        }
        return any_left ? Next::kWait : Next::kFinished;
    }

    // The task has issued its export: view v's depth map of passes[pi] may be read.
    void Publish(int pi, int v) { published_[v] = passes_[pi].iteration; }
    // The lane is done with the task (published or not: a failed run publishes nothing).  True: it was the last of its pass.
    // (>=: another lane may have taken and published the view's next pass since this task published.)
    bool Finish(int pi, int v)
    {
        --active_[pi];
        return published_[v] >= passes_[pi].iteration && --remaining_[pi] == 0;
    }

    int Published(int v) const { return published_[v]; }  // the newest iteration whose depth map view v has published
    // Which iteration of view j's depth map the task (passes[pi], v) reads: its own pass's when j precedes v in the reference's
    // order, the pass before otherwise (and for v itself).  The reader waits until Published(j) has reached it.
    int SourceIteration(int pi, int v, int j) const { return (gauss_seidel_ && j < v) ? passes_[pi].iteration : passes_[pi].iteration - 1; }

private:
    // Eligible: the view's own previous pass is done, the maps of the previous pass it will read are published and the last readers
    // of the map it will overwrite are done (so that a running task only ever waits for views of its OWN pass that went out before
    // it: no wait can point at a task nobody holds), and -- in the reference's order, where the second halves of a geometric pass
    // form a chain -- at most lanes_per_pass lanes work on one pass: one more would only queue up behind the chain, while the next
    // pass can already start its first views.  The smallest unfinished (pass, view) is always eligible or running, so the level
    // drains.
    bool Eligible(int pi, int v) const
    {
        const int it = passes_[pi].iteration;
        if (pi > 0 && published_[v] < it - 1) {
            return false;
        }
        if (it - 2 >= passes_[0].iteration) {  // the export will overwrite the view's map of pass it - 2: its last readers must be done
            for (int w : readers_[v]) {
                if (published_[w] < ((gauss_seidel_ && w > v) ? it - 2 : it - 1)) {
                    return false;
                }
            }
        }
        if (passes_[pi].geom_consistency) {
            if (gauss_seidel_ && active_[pi] >= lanes_per_pass_) {
                return false;
            }
            for (int u : sources_[v]) {
                if (!(gauss_seidel_ && u < v) && published_[u] < it - 1) {
                    return false;
                }
            }
        }
        return true;
    }

    std::vector<PassInfo> passes_;
    std::vector<std::vector<int>> sources_, readers_;  // readers_[u]: the views that list u as a source
    bool gauss_seidel_;
    int lanes_per_pass_;
    std::vector<int> published_;                      // per view
    std::vector<int> remaining_, frontier_, active_;  // per pass: unfinished views, next view to hand out, tasks running
};

#endif  // APD_MI355X_HOST_WAVEFRONT_H_
