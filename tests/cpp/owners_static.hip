// The owners of sampler_base.hpp: move-only, and they move without throwing (compiled by tests/test_resource_owners.py).
#include <type_traits>

#include "sampler_base.hpp"

using namespace mcmcpp;

template <class O>
constexpr bool move_only()
{
    return !std::is_copy_constructible<O>::value && !std::is_copy_assignable<O>::value && std::is_nothrow_move_constructible<O>::value &&
           std::is_nothrow_move_assignable<O>::value;
}
static_assert(move_only<DeviceBuffer<>>(), "DeviceBuffer");
static_assert(move_only<DeviceBuffer<double>>(), "DeviceBuffer<double>");
static_assert(move_only<PinnedBuffer<char>>(), "PinnedBuffer");
static_assert(move_only<Event>(), "Event");
static_assert(move_only<GraphExec>(), "GraphExec");
static_assert(move_only<Stream>(), "Stream");

int main() { return 0; }
