// The process-wide A/B knobs of ops.hip's dispatchers (fac_set_option, cvit_abi.hip),
// each defined beside the route it steers.
#pragma once

namespace fac {

void set_nd_pt_wide(int v);
void set_nd_occ3(int v);
void set_pool_roll(int v);
void set_pool_win(int v);
void set_pool3_zg(int v);
void set_pool_lds14(int v);
void set_pool3_g(int v);
void set_pw_res(int v);
void set_tk_wreg(int v);

}  // namespace fac
