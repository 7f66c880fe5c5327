// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the task graph.  Our own code; it holds no game logic.
//
// TaskGraphBuilder records the nodes in the order setupTasks adds them, with the dependencies each names
// (a dependency must already be in the graph, so insertion order is a topological order).  run()
// executes node by node; each node runs over the worlds in the order it is given them.
// ParallelForNode<Ctx, fn, Cs...> calls fn(ctx, Cs&...) on every entity of the world that has all of Cs;
// a singleton is a component of the world's singleton entity (entity 0).
//
// Madrona leaves open which topological order the nodes run in and in which order a node visits its
// entities.  run() therefore offers two of each, so that a test can show that the results do not depend
// on the choice:
//   graph_order 0       insertion order (the default; what every driver used before the options existed)
//   graph_order 1       of the nodes whose dependencies have all run, always the one added LAST.  For a
//                       graph with several independent chains this starts with the last root and runs
//                       later chains before earlier ones.
//   reverse_entities    a node visits its entities in descending instead of ascending creation order
#pragma once

#include <cstdint>
#include <initializer_list>
#include <vector>

#include "custom_context.hpp"

namespace madrona {

template <typename ContextT, auto Fn, typename FirstT, typename... ComponentTs>
struct ParallelForNode {
    static void run(void *ctx_ptr, bool reverse_entities)
    {
        ContextT &ctx = *static_cast<ContextT *>(ctx_ptr);
        standin::WorldStore &store = ctx.store();
        const std::vector<uint32_t> &with_first = store.entities_with<FirstT>();  // ascending
        const size_t n = with_first.size();
        for (size_t i = 0; i < n; i++) {
            const uint32_t e = with_first[reverse_entities ? n - 1 - i : i];
            if (((store.find<ComponentTs>(e) != nullptr) && ... && true))
                Fn(ctx, store.get<FirstT>(e), store.get<ComponentTs>(e)...);
        }
    }
};

class TaskGraphBuilder {
public:
    struct NodeID {
        uint32_t id;
    };

    template <typename NodeT>
    NodeID addToGraph(std::initializer_list<NodeID> deps)
    {
        std::vector<uint32_t> d;
        for (NodeID dep : deps) {
            if (dep.id >= nodes_.size()) __builtin_trap();  // a dependency must already be in the graph
            d.push_back(dep.id);
        }
        nodes_.push_back(&NodeT::run);
        deps_.push_back(d);
        return NodeID{(uint32_t)nodes_.size() - 1};
    }

    // The node ids in the order run() executes them for graph_order (see the top of the file).
    std::vector<uint32_t> order(int graph_order) const
    {
        const uint32_t n = (uint32_t)nodes_.size();
        std::vector<uint32_t> out;
        if (graph_order == 0) {
            for (uint32_t i = 0; i < n; i++) out.push_back(i);
            return out;
        }
        std::vector<bool> ran(n, false);
        while (out.size() < n) {
            for (uint32_t k = n; k-- > 0;) {
                if (ran[k]) continue;
                bool ready = true;
                for (uint32_t d : deps_[k]) ready = ready && ran[d];
                if (!ready) continue;
                ran[k] = true;
                out.push_back(k);
                break;
            }
        }
        return out;
    }

    // contexts: one per world, in the order the worlds are to run within each node
    template <typename ContextT>
    void run(const std::vector<ContextT *> &contexts, int graph_order = 0, bool reverse_entities = false) const
    {
        for (uint32_t k : order(graph_order))
            for (ContextT *ctx : contexts) nodes_[k](ctx, reverse_entities);
    }

private:
    std::vector<void (*)(void *, bool)> nodes_;
    std::vector<std::vector<uint32_t>> deps_;
};

}  // namespace madrona
