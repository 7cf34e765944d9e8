// fg_switch.h -- an environment switch as the launch plans (fg_hmc_sep_plan.h, fg_mh_mw_plan.h, fg_hmc_split_plan.h) take it: unset, or its integer value.
// The launchers read the environment (fg_env_switch); the plans only see the values.
#pragma once
#include <cstdlib>

struct FgSwitch { bool set; int v; };
inline FgSwitch fg_env_switch(const char *name) { const char *v = std::getenv(name); return FgSwitch{ v != nullptr, v ? std::atoi(v) : 0 }; }
inline bool fg_switch_is(const FgSwitch &s, int v) { return s.set && s.v == v; }
