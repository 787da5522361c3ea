// faiss::IndexIVF (IndexIVF.h:45-108): inverted-file base with the reference's
// public fields (drivers poke nprobe / quantizer_trains_alone / cp directly), and
// faiss::IndexIVFFlat (IndexIVF.h:132-205) over the MI355X library.
#pragma once
#include <vector>

#include "AuxIndexStructures.h"
#include "Clustering.h"
#include "Heap.h"
#include "Index.h"

namespace faiss {

struct IndexIVF : Index {
  size_t nlist;
  size_t nprobe;
  Index* quantizer;
  bool quantizer_trains_alone;
  bool own_fields;
  ClusteringParameters cp;
  std::vector<std::vector<long> > ids;
  bool maintain_direct_map;
  std::vector<long> direct_map;

  IndexIVF(Index* quantizer, size_t d, size_t nlist, MetricType metric = METRIC_INNER_PRODUCT)
      : Index(d, metric), nlist(nlist), nprobe(1), quantizer(quantizer), quantizer_trains_alone(false),
        own_fields(false), ids(nlist), maintain_direct_map(false) {
    FAISS_THROW_IF_NOT(d == (size_t)quantizer->d);
    is_trained = quantizer->is_trained && (quantizer->ntotal == (idx_t)nlist);
    cp.niter = 10;   // IndexIVF.cpp:51
  }
  IndexIVF() : nlist(0), nprobe(1), quantizer(nullptr), quantizer_trains_alone(false), own_fields(false),
               maintain_direct_map(false) {}
  ~IndexIVF() override { if (own_fields) delete quantizer; }

  void reset() override {
    ntotal = 0;
    direct_map.clear();
    for (auto& l : ids) l.clear();
  }
  /// IndexIVF::train (IndexIVF.cpp:102-129)
  void train(idx_t n, const float* x) override {
    if (quantizer->is_trained && quantizer->ntotal == (idx_t)nlist) {
      if (verbose) printf("IVF quantizer does not need training.\n");
    } else if (quantizer_trains_alone) {
      quantizer->train(n, x);
      FAISS_THROW_IF_NOT_MSG(quantizer->ntotal == (idx_t)nlist, "nlist not consistent with quantizer size");
    } else {
      if (verbose) printf("Training IVF quantizer on %ld vectors in %dD\n", n, d);
      Clustering clus(d, (int)nlist, cp);
      quantizer->reset();
      clus.train(n, x, *quantizer);
      quantizer->is_trained = true;
    }
    train_residual(n, x);
    is_trained = true;
  }
  void add(idx_t n, const float* x) override { add_with_ids(n, x, nullptr); }
  virtual void train_residual(idx_t, const float*) {}
  /// IndexIVF::merge_from (IndexIVF.cpp:150-177): moves the other index's lists into this one, `add_id` added to its ids
  virtual void merge_from_residuals(IndexIVF&) { FAISS_THROW_MSG("merge_from_residuals not implemented for this type of index"); }
  void merge_from(IndexIVF& other, idx_t add_id) {
    FAISS_THROW_IF_NOT(other.d == d && other.nlist == nlist);
    FAISS_THROW_IF_NOT_MSG(!maintain_direct_map && !other.maintain_direct_map, "direct map copy not implemented");
    FAISS_THROW_IF_NOT_MSG(typeid(*this) == typeid(other), "can only merge indexes of the same type");
    for (size_t i = 0; i < nlist; i++) {
      std::vector<long>& src = other.ids[i];
      std::vector<long>& dest = ids[i];
      for (size_t j = 0; j < src.size(); j++) dest.push_back(src[j] + add_id);
      src.clear();
    }
    merge_from_residuals(other);
    ntotal += other.ntotal;
    other.ntotal = 0;
  }
  size_t get_list_size(size_t list_no) const { return ids[list_no].size(); }
  /// 1 = perfectly balanced (IndexIVF.cpp:140-147)
  double imbalance_factor() const {
    double tot = 0, uf = 0;
    for (size_t i = 0; i < nlist; i++) { tot += ids[i].size(); uf += ids[i].size() * (double)ids[i].size(); }
    return tot > 0 ? uf * nlist / (tot * tot) : 0;
  }
};

struct IndexIVFFlatStats {   // IndexIVF.h:111-119
  size_t nq;        // nb of queries run
  size_t nlist;     // nb of inverted lists scanned
  size_t ndis;      // nb of distances computed
  size_t npartial;  // nb of bound computations (IndexIVFFlatIPBounds: not built)
  IndexIVFFlatStats() { reset(); }
  void reset() { memset((void*)this, 0, sizeof(*this)); }
};
inline IndexIVFFlatStats indexIVFFlat_stats;   // "global var that collects them all" (IndexIVF.h:122); C++17

/// faiss::IndexIVFFlat (IndexIVF.h:132-205, IndexIVF.cpp:200-582): the inverted lists hold the vectors themselves.  Same public
/// data model (ids / vecs per list); the host-side lists stay the authoritative copy -- what write_index and copyFrom read --
/// and are mirrored to the device list-contiguously before the first search after a change.  add_core assigns on the device
/// (the quantizer's 1-NN) and appends to the host lists; search, search_preassigned and range_search run on the device
/// (vlq_ivfflat_*).  update_vectors and IndexIVFFlatIPBounds are not built.
struct IndexIVFFlat : IndexIVF {
  std::vector<std::vector<float> > vecs;   ///< list i: an nl x d matrix

  /// device the index lives on (set before add/search)
  int device = 0;

  IndexIVFFlat(Index* quantizer, size_t d, size_t nlist_, MetricType metric = METRIC_INNER_PRODUCT)
      : IndexIVF(quantizer, d, nlist_, metric) {
    vecs.resize(nlist);
  }
  IndexIVFFlat() {}
  ~IndexIVFFlat() override { if (h_) vlq_ivfflat_destroy(h_); }
  IndexIVFFlat(const IndexIVFFlat&) = delete;
  IndexIVFFlat& operator=(const IndexIVFFlat&) = delete;

  void add_with_ids(idx_t n, const float* x, const long* xids) override { add_core(n, x, xids, nullptr); }

  /// add_core (IndexIVF.cpp:221-262): a negative list id drops the vector; ntotal grows by the vectors kept
  virtual void add_core(idx_t n, const float* x, const long* xids, const long* precomputed_idx) {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT_MSG(!(maintain_direct_map && xids), "cannot have direct map and add with ids");
    if (n == 0) return;
    std::vector<long> idx0;
    const long* idx = precomputed_idx;
    if (!idx) {
      idx0.resize(n);
      quantizer->assign(n, x, idx0.data());
      idx = idx0.data();
    }
    long n_add = 0;
    for (idx_t i = 0; i < n; i++) {
      const long id = xids ? xids[i] : ntotal + i;
      const long list_no = idx[i];
      if (list_no < 0) continue;
      FAISS_THROW_IF_NOT((size_t)list_no < nlist);
      ids[list_no].push_back(id);
      vecs[list_no].insert(vecs[list_no].end(), x + i * d, x + (i + 1) * d);
      if (maintain_direct_map) direct_map.push_back(list_no << 32 | (long)(ids[list_no].size() - 1));
      n_add++;
    }
    ntotal += n_add;
    ldirty_ = true;
  }

  /// IndexIVF.cpp:373-380: quantizer->assign with nprobe, then search_preassigned -- both stages in one device call
  void search(idx_t n, const float* x, idx_t k, float* distances, idx_t* labels) const override {
    sync_();
    VLQ_CHECK(vlq_ivfflat_search(h_, n, x, (int)nprobe, (int)k, distances, (int64_t*)labels));
    collect_stats_();
  }

  /// IndexIVF.cpp:383-398: assign [n][nprobe]
  void search_preassigned(idx_t n, const float* x, idx_t k, const idx_t* assign, float* distances, idx_t* labels) const {
    sync_();
    VLQ_CHECK(vlq_ivfflat_search_preassigned(h_, n, x, (const int64_t*)assign, (int)nprobe, (int)k, distances, (int64_t*)labels));
    collect_stats_();
  }

  /// IndexIVF.cpp:401-449: quantizer->assign with nprobe, then every stored vector of those lists with dis < radius (L2) or
  /// ip > radius (inner product), per query in scan order (probe order, then list position) -- one device call.  The counts go
  /// through result->do_allocation() as in the reference, so an overloaded allocation is honoured.  indexIVFFlat_stats is
  /// not touched (the reference's range_search keeps no statistics).
  void range_search(idx_t n, const float* x, float radius, RangeSearchResult* result) const override {
    FAISS_THROW_IF_NOT_MSG(result && (idx_t)result->nq == n, "RangeSearchResult must be constructed for the n queries");
    sync_();
    std::vector<int64_t> lims((size_t)n + 1, 0);
    VLQ_CHECK(vlq_ivfflat_range_search(h_, n, x, (int)nprobe, radius, lims.data(), nullptr));
    for (idx_t i = 0; i < n; i++) result->lims[i] = (size_t)(lims[i + 1] - lims[i]);
    result->do_allocation();
    VLQ_CHECK(vlq_ivfflat_range_result(h_, result->distances, (int64_t*)result->labels));
  }

  void reset() override {   // IndexIVF.cpp:533-539
    IndexIVF::reset();
    for (auto& v : vecs) v.clear();
    ldirty_ = true;
  }

  /// IndexIVF.cpp:541-570: a removed entry is replaced by the list's last one
  long remove_ids(const IDSelector& sel) override {
    FAISS_THROW_IF_NOT_MSG(!maintain_direct_map, "direct map remove not implemented");
    long nremove = 0;
    for (size_t i = 0; i < nlist; i++) {
      std::vector<long>& idsi = ids[i];
      float* vecsi = vecs[i].data();
      long l = (long)idsi.size(), j = 0;
      while (j < l) {
        if (sel.is_member(idsi[j])) {
          l--;
          idsi[j] = idsi[l];
          memmove(vecsi + j * d, vecsi + l * d, d * sizeof(float));
        } else {
          j++;
        }
      }
      if (l < (long)idsi.size()) {
        nremove += (long)idsi.size() - l;
        idsi.resize(l);
        vecs[i].resize((size_t)l * d);
      }
    }
    ntotal -= nremove;
    if (nremove) ldirty_ = true;
    return nremove;
  }

  /// IndexIVF.cpp:573-580
  void reconstruct(idx_t key, float* recons) const override {
    FAISS_THROW_IF_NOT_MSG(direct_map.size() == (size_t)ntotal, "direct map is not initialized");
    FAISS_THROW_IF_NOT(key >= 0 && key < ntotal);
    const long list_no = direct_map[key] >> 32, ofs = direct_map[key] & 0xffffffff;
    memcpy(recons, &vecs[list_no][ofs * d], d * sizeof(recons[0]));
  }

  /// IndexIVF::make_direct_map (IndexIVF.cpp:68-90)
  void make_direct_map(bool new_maintain_direct_map = true) {
    if (new_maintain_direct_map == maintain_direct_map) return;
    if (new_maintain_direct_map) {
      direct_map.assign(ntotal, -1);
      for (size_t key = 0; key < nlist; key++)
        for (size_t ofs = 0; ofs < ids[key].size(); ofs++) {
          FAISS_THROW_IF_NOT_MSG(0 <= ids[key][ofs] && ids[key][ofs] < ntotal, "direct map supported only for sequential ids");
          direct_map[ids[key][ofs]] = (long)key << 32 | (long)ofs;
        }
    } else {
      direct_map.clear();
    }
    maintain_direct_map = new_maintain_direct_map;
  }

  /// moves the other index's vectors behind this one's (IndexIVF.cpp:451-461; the ids move in IndexIVF::merge_from)
  void merge_from_residuals(IndexIVF& other_in) override {
    IndexIVFFlat& other = dynamic_cast<IndexIVFFlat&>(other_in);
    for (size_t i = 0; i < nlist; i++) {
      vecs[i].insert(vecs[i].end(), other.vecs[i].begin(), other.vecs[i].end());
      other.vecs[i].clear();
    }
    ldirty_ = other.ldirty_ = true;
  }

  /// copies the entries with a1 <= id < a2 (subset_type 0).  IndexIVF.h:166-172 also documents subset_type 1 (id % a1 == a2),
  /// but the reference's loop (IndexIVF.cpp:463-486) copies nothing for it; the same happens here
  void copy_subset_to(IndexIVFFlat& other, int subset_type, long a1, long a2) const {
    FAISS_THROW_IF_NOT(nlist == other.nlist);
    FAISS_THROW_IF_NOT(!other.maintain_direct_map);
    for (size_t list_no = 0; list_no < nlist; list_no++) {
      const std::vector<long>& ids_in = ids[list_no];
      const std::vector<float>& vecs_in = vecs[list_no];
      for (size_t i = 0; i < ids_in.size(); i++) {
        const long id = ids_in[i];
        if (subset_type == 0 && a1 <= id && id < a2) {
          other.ids[list_no].push_back(id);
          other.vecs[list_no].insert(other.vecs[list_no].end(), vecs_in.begin() + i * d, vecs_in.begin() + (i + 1) * d);
          other.ntotal++;
        }
      }
    }
    other.ldirty_ = true;
  }

  /// after writing ids / vecs / the quantizer directly (read_index, a copy from another index)
  void lists_changed() { ldirty_ = hdirty_ = true; }

 protected:
  void collect_stats_() const {
    uint64_t nq = 0, nl = 0, nd = 0;
    VLQ_CHECK(vlq_ivfflat_stats(h_, &nq, &nl, &nd, 1));   // also raises on an invalid key (IndexIVF.cpp:296-300, :346-350)
    indexIVFFlat_stats.nq += nq;
    indexIVFFlat_stats.nlist += nl;
    indexIVFFlat_stats.ndis += nd;
  }
  void sync_() const {
    FAISS_THROW_IF_NOT(is_trained);
    FAISS_THROW_IF_NOT_MSG(metric_type == METRIC_L2 || metric_type == METRIC_INNER_PRODUCT, "unknown metric");
    FAISS_THROW_IF_NOT_MSG(quantizer && quantizer->ntotal == (idx_t)nlist && quantizer->metric_type == metric_type,
                           "coarse quantizer must be an IndexFlatL2 / IndexFlatIP of nlist vectors with the index's metric");
    if (!h_) {
      VLQ_CHECK(vlq_ivfflat_create(&h_, device, d, (int)nlist, (int)metric_type));
      hdirty_ = ldirty_ = true;
    }
    if (hdirty_) {
      std::vector<float> cent((size_t)nlist * d);     // (IndexFlat::xb, through the Index interface: IndexIVF.h precedes IndexFlat.h)
      quantizer->reconstruct_n(0, (idx_t)nlist, cent.data());
      VLQ_CHECK(vlq_ivfflat_set_coarse_centroids(h_, cent.data()));
      hdirty_ = false;
    }
    if (ldirty_) {
      std::vector<int64_t> off(nlist + 1, 0);
      for (size_t i = 0; i < nlist; i++) off[i + 1] = off[i] + (int64_t)ids[i].size();
      std::vector<float> fv((size_t)off[nlist] * d);
      std::vector<int64_t> fi((size_t)off[nlist]);
      for (size_t i = 0; i < nlist; i++) {
        if (ids[i].empty()) continue;
        FAISS_THROW_IF_NOT(vecs[i].size() == ids[i].size() * (size_t)d);
        memcpy(&fv[(size_t)off[i] * d], vecs[i].data(), vecs[i].size() * sizeof(float));
        for (size_t j = 0; j < ids[i].size(); j++) fi[off[i] + j] = ids[i][j];
      }
      VLQ_CHECK(vlq_ivfflat_set_lists(h_, fv.data(), fi.data(), off.data()));
      ldirty_ = false;
    }
  }
  mutable vlq_ivfflat_t h_ = nullptr;
  mutable bool hdirty_ = true, ldirty_ = true;
};

}  // namespace faiss
