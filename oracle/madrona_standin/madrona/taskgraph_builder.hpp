// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the task graph.  Our own code; it holds no game logic.
//
// TaskGraphBuilder records the nodes in the order setupTasks adds them (which, for the three sim files
// built against this stand-in, is also their dependency order).  run() executes node by node; each node
// runs over the worlds in the order it is given them.  ParallelForNode<Ctx, fn, Cs...> calls
// fn(ctx, Cs&...) on every entity of the world, in creation order, that has all of Cs; a singleton is a
// component of the world's singleton entity (entity 0).
#pragma once

#include <cstdint>
#include <initializer_list>
#include <vector>

#include "custom_context.hpp"

namespace madrona {

template <typename ContextT, auto Fn, typename... ComponentTs>
struct ParallelForNode {
    static void run(void *ctx_ptr)
    {
        ContextT &ctx = *static_cast<ContextT *>(ctx_ptr);
        standin::WorldStore &store = ctx.store();
        const uint32_t n = store.num_entities();
        for (uint32_t e = 0; e < n; e++) {
            if (((store.find<ComponentTs>(e) != nullptr) && ...))
                Fn(ctx, store.get<ComponentTs>(e)...);
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
        for (NodeID d : deps)
            if (d.id >= nodes_.size()) __builtin_trap();  // a dependency must already be in the graph
        nodes_.push_back(&NodeT::run);
        return NodeID{(uint32_t)nodes_.size() - 1};
    }

    // contexts: one per world, in the order the worlds are to run within each node
    template <typename ContextT>
    void run(const std::vector<ContextT *> &contexts) const
    {
        for (auto node : nodes_)
            for (ContextT *ctx : contexts) node(ctx);
    }

private:
    std::vector<void (*)(void *)> nodes_;
};

}  // namespace madrona
