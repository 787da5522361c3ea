// faiss::RangeSearchResult (AuxIndexStructures.h:29-48): what range_search() fills; faiss::IDSelector and its two stock
// implementations (AuxIndexStructures.h:52-88): what remove_ids() takes.  RangeSearchPartialResult / BufferList, the
// reference's per-thread buffers of a host-side range search, have no counterpart: the device call returns whole arrays.
#pragma once
#include <cstring>
#include <unordered_set>

#include "Index.h"

namespace faiss {

/// The result of a range search: query i's hits are labels / distances [lims[i] .. lims[i+1]), not sorted.
struct RangeSearchResult {
  size_t nq;      ///< nb of queries
  size_t* lims;   ///< size (nq + 1), zeroed; allocated on input to range_search

  typedef Index::idx_t idx_t;

  idx_t* labels;
  float* distances;

  size_t buffer_size;   ///< size of the result buffers used (of the reference's partial results; kept for layout)

  explicit RangeSearchResult(size_t nq) : nq(nq), labels(nullptr), distances(nullptr), buffer_size(1024 * 256) {
    lims = new size_t[nq + 1];
    memset(lims, 0, sizeof(*lims) * (nq + 1));
  }
  RangeSearchResult(const RangeSearchResult&) = delete;
  RangeSearchResult& operator=(const RangeSearchResult&) = delete;

  /// called when lims holds the number of result entries of each query: turns them into offsets (lims[nq] = the total)
  /// and allocates labels and distances.  Can be overloaded to allocate the tables elsewhere.
  virtual void do_allocation() {
    size_t ofs = 0;
    for (size_t i = 0; i < nq; i++) {
      const size_t n = lims[i];
      lims[i] = ofs;
      ofs += n;
    }
    lims[nq] = ofs;
    labels = new idx_t[ofs];
    distances = new float[ofs];
  }

  virtual ~RangeSearchResult() {
    delete[] labels;
    delete[] distances;
    delete[] lims;
  }
};

struct IDSelector {
  typedef Index::idx_t idx_t;
  virtual bool is_member(idx_t id) const = 0;
  virtual ~IDSelector() {}
};

/// ids in [imin, imax)
struct IDSelectorRange : IDSelector {
  idx_t imin, imax;
  IDSelectorRange(idx_t imin, idx_t imax) : imin(imin), imax(imax) {}
  bool is_member(idx_t id) const override { return id >= imin && id < imax; }
};

/// an explicit set of ids (the reference pairs a hash set with a Bloom filter for speed; membership is the same)
struct IDSelectorBatch : IDSelector {
  std::unordered_set<idx_t> set;
  IDSelectorBatch(long n, const idx_t* indices) : set(indices, indices + n) {}
  bool is_member(idx_t id) const override { return set.count(id) != 0; }
};

}  // namespace faiss
