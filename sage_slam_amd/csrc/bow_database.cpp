// bow_database.cpp -- host side of the loop detector's retrieval (no HIP): the L1 score of two bag-of-words vectors
// (L1Scoring::score, DBoW2/src/ScoringObject.cpp:23-68) and the inverted-file database (TemplatedDatabase::add / queryL1,
// DBoW2/include/DBoW2/TemplatedDatabase.h:604-675).  A vector is two parallel arrays: strictly ascending word ids and their
// values.  Sums run in the reference's order (ascending word id), so the scores are its doubles bit for bit; where its
// std::sort leaves the order of tied values open, ties go by ascending entry id here.
#include "sage_ba.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <utility>
#include <vector>

namespace
{
// strictly ascending ids in [0, n_words) (n_words < 0: any non-negative id), finite values
bool bow_vector_ok(const int32_t *ids, const double *vals, int n, int n_words)
{
  if (n < 0 || (n > 0 && (!ids || !vals)))
    return false;
  for (int k = 0; k < n; ++k)
  {
    if (ids[k] < 0 || (n_words >= 0 && ids[k] >= n_words) || (k > 0 && ids[k] <= ids[k - 1]) || !std::isfinite(vals[k]))
      return false;
  }
  return true;
}

inline double l1_term(double v, double w) { return std::fabs(v - w) - std::fabs(v) - std::fabs(w); }
} // namespace

struct SageBowDatabase
{
  struct Item // one entry of a word's row
  {
    int32_t entry;
    double value;
  };
  int n_words = 0;
  int n_entries = 0;
  std::vector<std::vector<Item>> rows; // [n_words]: ascending entry ids (entries are appended in the order they come)
  mutable std::mutex mu;
};

extern "C" int sage_bow_score(const int32_t *ids1, const double *vals1, int n1, const int32_t *ids2, const double *vals2, int n2,
                              double *score)
{
  if (!score || !bow_vector_ok(ids1, vals1, n1, -1) || !bow_vector_ok(ids2, vals2, n2, -1))
    return SAGE_E_INVALID;
  double s = 0.0;
  for (int a = 0, b = 0; a < n1 && b < n2;)
  {
    if (ids1[a] == ids2[b])
    {
      s += l1_term(vals1[a], vals2[b]);
      ++a;
      ++b;
    }
    else if (ids1[a] < ids2[b])
      ++a;
    else
      ++b;
  }
  *score = -s / 2.0;
  return SAGE_OK;
}

extern "C" int sage_bow_db_create(int n_words, SageBowDatabase **out)
{
  if (!out || n_words < 1)
    return SAGE_E_INVALID;
  SageBowDatabase *db = new SageBowDatabase();
  db->n_words = n_words;
  db->rows.resize((size_t)n_words);
  *out = db;
  return SAGE_OK;
}

extern "C" void sage_bow_db_destroy(SageBowDatabase *db) { delete db; }

extern "C" int sage_bow_db_add(SageBowDatabase *db, const int32_t *ids, const double *vals, int n)
{
  if (!db || !bow_vector_ok(ids, vals, n, db->n_words))
    return SAGE_E_INVALID;
  std::lock_guard<std::mutex> lock(db->mu);
  const int32_t entry = db->n_entries++;
  for (int k = 0; k < n; ++k)
    db->rows[(size_t)ids[k]].push_back(SageBowDatabase::Item{entry, vals[k]});
  return entry;
}

extern "C" int sage_bow_db_size(const SageBowDatabase *db)
{
  if (!db)
    return -1;
  std::lock_guard<std::mutex> lock(db->mu);
  return db->n_entries;
}

extern "C" int sage_bow_db_query(const SageBowDatabase *db, const int32_t *ids, const double *vals, int n, int max_results,
                                 int max_id, int32_t *entry_ids, double *scores, int capacity, int *n_out)
{
  if (!db || !n_out || capacity < 0 || (capacity > 0 && (!entry_ids || !scores)) || !bow_vector_ok(ids, vals, n, db->n_words))
    return SAGE_E_INVALID;
  std::vector<std::pair<double, int32_t>> found; // (accumulated value, entry)
  {
    std::lock_guard<std::mutex> lock(db->mu);
    std::vector<double> acc((size_t)db->n_entries, 0.0);
    std::vector<char> touched((size_t)db->n_entries, 0);
    for (int k = 0; k < n; ++k) // the query's words in ascending order: every entry's sum runs in the reference's order
      for (const SageBowDatabase::Item &it : db->rows[(size_t)ids[k]])
        if (it.entry < max_id || max_id == -1)
        {
          const double term = l1_term(vals[k], it.value);
          acc[(size_t)it.entry] = touched[(size_t)it.entry] ? acc[(size_t)it.entry] + term : term;
          touched[(size_t)it.entry] = 1;
        }
    for (int e = 0; e < db->n_entries; ++e)
      if (touched[(size_t)e])
        found.emplace_back(acc[(size_t)e], e);
  }
  std::sort(found.begin(), found.end()); // ascending value (the lower the better); equal values: ascending entry id
  if (max_results > 0 && (int)found.size() > max_results)
    found.resize((size_t)max_results);
  *n_out = (int)found.size();
  if ((int)found.size() > capacity)
    return SAGE_E_INVALID;
  for (size_t k = 0; k < found.size(); ++k)
  {
    entry_ids[k] = found[k].second;
    scores[k] = -found[k].first / 2.0;
  }
  return SAGE_OK;
}
