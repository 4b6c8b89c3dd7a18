// gx_sparse.h -- sparse lists on the host: keys ascending, K columns of sums beside them (the complexity's multiplicities, the
// interval lengths, the depth's deep list).  Two operations: append an entry to a list that is being read back in ascending order,
// folding a key that repeats; add one list to another.  Host only, nothing of the library's: tests/sparse_main.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace gx_sparse {

using Col = std::vector<uint64_t>;

// (k, v[0..K)) at the end of the list; k is not below the last key, and a k equal to it adds to its sums
template <size_t K>
void append(Col& key, Col* const (&val)[K], uint64_t k, const uint64_t (&v)[K]) {
  const bool fold = !key.empty() && key.back() == k;
  if (!fold) key.push_back(k);
  for (size_t c = 0; c < K; c++) {
    if (fold) val[c]->back() += v[c];
    else val[c]->push_back(v[c]);
  }
}

// b added to a: the keys of both ascending and distinct; a key of both adds its sums
template <size_t K>
void add(Col& aKey, Col* const (&aVal)[K], const Col& bKey, const Col* const (&bVal)[K]) {
  Col key, val[K];
  Col* out[K];
  for (size_t c = 0; c < K; c++) out[c] = &val[c];
  size_t i = 0, j = 0;
  while (i < aKey.size() || j < bKey.size()) {
    const bool fromA = j == bKey.size() || (i < aKey.size() && aKey[i] <= bKey[j]);
    uint64_t v[K];
    for (size_t c = 0; c < K; c++) v[c] = fromA ? (*aVal[c])[i] : (*bVal[c])[j];
    append(key, out, fromA ? aKey[i++] : bKey[j++], v);
  }
  aKey = std::move(key);
  for (size_t c = 0; c < K; c++) *aVal[c] = std::move(val[c]);
}

}  // namespace gx_sparse
