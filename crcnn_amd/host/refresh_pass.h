// refresh_pass.h -- how many items one pass of a client-side refresh takes (refreshImages, rescaleSlots, actSlots, rescaleSlotsCrt), header only: no engine, no
// device.  An item is a ciphertext, or for actSlots a whole plane of in_cts_per_item input ciphertexts.  A pass takes what 4 GiB of work space hold
// (one_item_bytes = the work of one item), at least 1024 input ciphertexts' worth of items, at most every item.
#pragma once
#include <algorithm>
#include <cstddef>

inline size_t refresh_pass_len(size_t one_item_bytes, size_t items, size_t in_cts_per_item)
{
    const size_t budget = ((size_t)4 << 30) / std::max<size_t>(one_item_bytes, 1), in_cts = std::max<size_t>(in_cts_per_item, 1);
    return std::min(items, std::max(budget, (1024 + in_cts - 1) / in_cts));
}
