// encode.cpp — host encoder for the MI355X provisioning solve: the driver.
//
// Turns gs_problem (what Go's GetInstanceTypes + NewScheduler inputs carry,
// reference pkg/cloudprovider/cloudprovider.go:553-583) into the bitset/SoA
// layout of layout.hpp, phase by phase (encode_ctx.hpp; one encode_*.cpp per
// phase family, the requirement algebra in reqs.cpp, the threads in par.cpp).
#include "encode.hpp"

#include <memory>
#include <stdexcept>

#include "encode_ctx.hpp"

namespace gsh {

Err encode(const gs_problem* p, Encoded& e, uint32_t bound_alias) {
  enc::PhaseTimer tm;
  // the per-pod arrays keep their capacity across the prepares of one
  // context: a repeated Solve of a similar batch refills mapped memory
  // instead of faulting in fresh pages (~13 MB of variant records at CM)
  auto vars = std::move(e.vars);
  auto pod_req = std::move(e.pod_req);
  auto var_begin = std::move(e.var_begin), var_count = std::move(e.var_count), var_sv = std::move(e.var_sv),
       var_itclass = std::move(e.var_itclass), queue0 = std::move(e.queue0);
  e = Encoded();
  for (auto* v : {&var_begin, &var_count, &var_sv, &var_itclass, &queue0}) v->clear();
  vars.clear();
  pod_req.clear();
  e.vars = std::move(vars);
  e.pod_req = std::move(pod_req);
  e.var_begin = std::move(var_begin);
  e.var_count = std::move(var_count);
  e.var_sv = std::move(var_sv);
  e.var_itclass = std::move(var_itclass);
  e.queue0 = std::move(queue0);
  tm.phase("reset");
  Err r{};
  // the encoder's scratch (strings, maps, per-spec tables: ~10^5 heap blocks
  // at CM) is freed on a pool worker after encode returns, off the Solve's
  // critical path
  std::shared_ptr<enc::Ctx> cp(new enc::Ctx{p, e, tm, bound_alias});
  {
    enc::Ctx& c = *cp;
    try {
      c.strs.resize(p->n_strings);
      par_for(p->n_strings, 4096, [&](uint32_t i) {
        if (p->strings[i]) c.strs[i] = p->strings[i];
      });
      tm.phase("strings");
      c.build_canon();
      tm.phase("canon");
      c.build_vocab();
      tm.phase("vocab");
      c.build_catalog();
      tm.phase("catalog");
      c.build_templates();
      tm.phase("templates");
      c.number_free_keys();
      c.choose_shadow_keys();
      c.build_free_slots();
      tm.phase("free_slots");
      c.build_pods();
      tm.phase("pods");
      c.build_nodes();
      // every taint is known now (NodePools', then nodes'): the class masks
      c.build_taint_classes();
      tm.phase("nodes");
      c.build_topology();
      tm.phase("topology");
      c.build_volumes();
      tm.phase("volumes");
    } catch (const enc::Fail& f) {
      r = Err{f.code, f.msg};
    } catch (const std::out_of_range& ex) {
      r = Err{GS_E_INVALID, std::string("unknown vocabulary value: ") + ex.what()};
    }
  }
  run_detached([cp]() mutable { cp.reset(); });
  cp.reset();
  tm.phase("teardown");
  return r;
}

}  // namespace gsh
