// resident_match.cpp — the one registry behind pr_gist_flagged_count / pr_delight_flagged_count (resident_match.hpp).
#include "resident_match.hpp"

#include <map>
#include <mutex>
#include <utility>

namespace pr {
namespace resident {

namespace {
std::mutex g_last_mu;
std::map<std::pair<Kind, const pr_ctx*>, LastCall> g_last;
}  // namespace

void remember(Kind kind, const pr_ctx* ctx, const Db* db, int32_t m) {
  std::lock_guard<std::mutex> lk(g_last_mu);
  g_last[{kind, ctx}] = LastCall{db, m};
}

LastCall last_call(Kind kind, const pr_ctx* ctx) {
  std::lock_guard<std::mutex> lk(g_last_mu);
  auto it = g_last.find({kind, ctx});
  return it != g_last.end() ? it->second : LastCall{nullptr, 0};
}

void forget(const Db* db) {
  std::lock_guard<std::mutex> lk(g_last_mu);
  for (auto it = g_last.begin(); it != g_last.end();) it = it->second.db == db ? g_last.erase(it) : std::next(it);
}

}  // namespace resident
}  // namespace pr
