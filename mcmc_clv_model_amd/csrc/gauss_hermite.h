// Gauss-Hermite rules (weight exp(-t^2)) of the orders csrc/marginal.hip supports: per order Q the
// nodes t_j ascending, the weights w_j and c_j = log(w_j) + t_j^2, rounded once from 40 digits.
// Written by tools/make_gauss_hermite.py; do not edit.  tests/test_marginal_cpu.py checks it against
// numpy's hermgauss and the monomials up to degree 2 Q - 1.
#pragma once

#define CLV_GH_ORDERS {8, 16, 24, 32}
#define CLV_GH_N_ORDERS 4
#define CLV_GH_TOTAL 80  // entries of each table: the orders' rules one after another

// nodes
#define CLV_GH_T_INIT { \
  /* Q = 8 */ \
  -0x1.771f208238266p+1, \
  -0x1.fb4ddb71e7f48p+0, \
  -0x1.283dd8de18830p+0, \
  -0x1.8655e1e2678c3p-2, \
  0x1.8655e1e2678c3p-2, \
  0x1.283dd8de18830p+0, \
  0x1.fb4ddb71e7f48p+0, \
  0x1.771f208238266p+1, \
  /* Q = 16 */ \
  -0x1.2c144c7cf336dp+2, \
  -0x1.ef4a11a67997ep+1, \
  -0x1.96a7e8960fc8ep+1, \
  -0x1.45e9f3ca7ad2fp+1, \
  -0x1.f3a860b5b5faap+0, \
  -0x1.61589fa5e2491p+0, \
  -0x1.a559e4708b514p-1, \
  -0x1.180b6a54f4f93p-2, \
  0x1.180b6a54f4f93p-2, \
  0x1.a559e4708b514p-1, \
  0x1.61589fa5e2491p+0, \
  0x1.f3a860b5b5faap+0, \
  0x1.45e9f3ca7ad2fp+1, \
  0x1.96a7e8960fc8ep+1, \
  0x1.ef4a11a67997ep+1, \
  0x1.2c144c7cf336dp+2, \
  /* Q = 24 */ \
  -0x1.8104eca55f9d9p+2, \
  -0x1.5099bad9de662p+2, \
  -0x1.280adbcd4a959p+2, \
  -0x1.036f3cd15e591p+2, \
  -0x1.c28f954fd719ap+1, \
  -0x1.819b1ca144820p+1, \
  -0x1.430e887d87971p+1, \
  -0x1.0645bfc521cedp+1, \
  -0x1.959168a1c4a36p+0, \
  -0x1.2073659e0df4fp+0, \
  -0x1.592cf49144110p-1, \
  -0x1.cb99dab120f5dp-3, \
  0x1.cb99dab120f5dp-3, \
  0x1.592cf49144110p-1, \
  0x1.2073659e0df4fp+0, \
  0x1.959168a1c4a36p+0, \
  0x1.0645bfc521cedp+1, \
  0x1.430e887d87971p+1, \
  0x1.819b1ca144820p+1, \
  0x1.c28f954fd719ap+1, \
  0x1.036f3cd15e591p+2, \
  0x1.280adbcd4a959p+2, \
  0x1.5099bad9de662p+2, \
  0x1.8104eca55f9d9p+2, \
  /* Q = 32 */ \
  -0x1.c80d55c906b62p+2, \
  -0x1.9a3537b9b8afap+2, \
  -0x1.73fb828c88899p+2, \
  -0x1.51a2a09addd6fp+2, \
  -0x1.31bd102f89f77p+2, \
  -0x1.138e1900c0335p+2, \
  -0x1.ed47dc1870b2ep+1, \
  -0x1.b565be914e170p+1, \
  -0x1.7f09f0797b8d8p+1, \
  -0x1.49e3501718808p+1, \
  -0x1.15b2263524badp+1, \
  -0x1.c484facec8d21p+0, \
  -0x1.5ed0fd0c409ffp+0, \
  -0x1.f3f7de674b058p-1, \
  -0x1.2b825634cdb6cp-1, \
  -0x1.8f08a9a7c06cfp-3, \
  0x1.8f08a9a7c06cfp-3, \
  0x1.2b825634cdb6cp-1, \
  0x1.f3f7de674b058p-1, \
  0x1.5ed0fd0c409ffp+0, \
  0x1.c484facec8d21p+0, \
  0x1.15b2263524badp+1, \
  0x1.49e3501718808p+1, \
  0x1.7f09f0797b8d8p+1, \
  0x1.b565be914e170p+1, \
  0x1.ed47dc1870b2ep+1, \
  0x1.138e1900c0335p+2, \
  0x1.31bd102f89f77p+2, \
  0x1.51a2a09addd6fp+2, \
  0x1.73fb828c88899p+2, \
  0x1.9a3537b9b8afap+2, \
  0x1.c80d55c906b62p+2, \
}

// weights
#define CLV_GH_W_INIT { \
  /* Q = 8 */ \
  0x1.a2999ecb217f6p-13, \
  0x1.17ce409fe72bfp-6, \
  0x1.a994440b42f6cp-3, \
  0x1.5281dc79924d8p-1, \
  0x1.5281dc79924d8p-1, \
  0x1.a994440b42f6cp-3, \
  0x1.17ce409fe72bfp-6, \
  0x1.a2999ecb217f6p-13, \
  /* Q = 16 */ \
  0x1.23e62febce393p-32, \
  0x1.f26d457674892p-23, \
  0x1.c6f9810be5860p-16, \
  0x1.e8c90a9ef9aa7p-11, \
  0x1.a60fe26755d4fp-7, \
  0x1.574932ae292a7p-4, \
  0x1.1f620c20579f4p-2, \
  0x1.040f552a19f20p-1, \
  0x1.040f552a19f20p-1, \
  0x1.1f620c20579f4p-2, \
  0x1.574932ae292a7p-4, \
  0x1.a60fe26755d4fp-7, \
  0x1.e8c90a9ef9aa7p-11, \
  0x1.c6f9810be5860p-16, \
  0x1.f26d457674892p-23, \
  0x1.23e62febce393p-32, \
  /* Q = 24 */ \
  0x1.7fc6f99c0742fp-53, \
  0x1.72ae60e3aadf0p-41, \
  0x1.4ef06f5a30c7fp-32, \
  0x1.593a1c5b7b34ep-25, \
  0x1.21acc1fc2fa1cp-19, \
  0x1.dd33b9015ae9fp-15, \
  0x1.afda22336bb7cp-11, \
  0x1.cdebc9b1e09f4p-8, \
  0x1.32c0d7e63b0dcp-5, \
  0x1.059c59cfbea66p-3, \
  0x1.250c3f8463c9ap-2, \
  0x1.b52d7169d64d8p-2, \
  0x1.b52d7169d64d8p-2, \
  0x1.250c3f8463c9ap-2, \
  0x1.059c59cfbea66p-3, \
  0x1.32c0d7e63b0dcp-5, \
  0x1.cdebc9b1e09f4p-8, \
  0x1.afda22336bb7cp-11, \
  0x1.dd33b9015ae9fp-15, \
  0x1.21acc1fc2fa1cp-19, \
  0x1.593a1c5b7b34ep-25, \
  0x1.4ef06f5a30c7fp-32, \
  0x1.72ae60e3aadf0p-41, \
  0x1.7fc6f99c0742fp-53, \
  /* Q = 32 */ \
  0x1.6185ca6732db3p-74, \
  0x1.1079077446a10p-60, \
  0x1.591c6504e6094p-50, \
  0x1.da9165dac4be2p-42, \
  0x1.04f2ec4d99a29p-34, \
  0x1.19ab6b0289e1dp-28, \
  0x1.520cca23243e8p-23, \
  0x1.e9f926629737dp-19, \
  0x1.c66041cb42acep-15, \
  0x1.1928b8bc0d2e1p-11, \
  0x1.df0dc4d8ce1d3p-9, \
  0x1.1f986ab0e9d28p-6, \
  0x1.ef45e3e774296p-5, \
  0x1.35cce805ded09p-3, \
  0x1.1c1dfcbccb09fp-2, \
  0x1.803e7b925d2ffp-2, \
  0x1.803e7b925d2ffp-2, \
  0x1.1c1dfcbccb09fp-2, \
  0x1.35cce805ded09p-3, \
  0x1.ef45e3e774296p-5, \
  0x1.1f986ab0e9d28p-6, \
  0x1.df0dc4d8ce1d3p-9, \
  0x1.1928b8bc0d2e1p-11, \
  0x1.c66041cb42acep-15, \
  0x1.e9f926629737dp-19, \
  0x1.520cca23243e8p-23, \
  0x1.19ab6b0289e1dp-28, \
  0x1.04f2ec4d99a29p-34, \
  0x1.da9165dac4be2p-42, \
  0x1.591c6504e6094p-50, \
  0x1.1079077446a10p-60, \
  0x1.6185ca6732db3p-74, \
}

// log(w) + t^2
#define CLV_GH_C_INIT { \
  /* Q = 8 */ \
  0x1.1c8307726c834p-4, \
  -0x1.24de118c3aa06p-3, \
  -0x1.db47e4bb61c8ep-3, \
  -0x1.12eb4008bac58p-2, \
  -0x1.12eb4008bac58p-2, \
  -0x1.db47e4bb61c8ep-3, \
  -0x1.24de118c3aa06p-3, \
  0x1.1c8307726c834p-4, \
  /* Q = 16 */ \
  -0x1.0b15654cf6c36p-4, \
  -0x1.36c31e0418498p-2, \
  -0x1.b0181ea3b722bp-2, \
  -0x1.fa99e14aa9de1p-2, \
  -0x1.15ccea7b3b784p-1, \
  -0x1.25eef833914f8p-1, \
  -0x1.2fd307a9f3bccp-1, \
  -0x1.348ab5f5c4810p-1, \
  -0x1.348ab5f5c4810p-1, \
  -0x1.2fd307a9f3bccp-1, \
  -0x1.25eef833914f8p-1, \
  -0x1.15ccea7b3b784p-1, \
  -0x1.fa99e14aa9de1p-2, \
  -0x1.b0181ea3b722bp-2, \
  -0x1.36c31e0418498p-2, \
  -0x1.0b15654cf6c36p-4, \
  /* Q = 24 */ \
  -0x1.1fdb7cb3451c8p-3, \
  -0x1.8d11287aaa09bp-2, \
  -0x1.07c5f850bf06cp-1, \
  -0x1.31e63d504db59p-1, \
  -0x1.4fc0ad0d5b772p-1, \
  -0x1.65e4c37efca36p-1, \
  -0x1.76a659f3fa77dp-1, \
  -0x1.8359e69445b7bp-1, \
  -0x1.8ccf9bc4dd0e7p-1, \
  -0x1.938b320549661p-1, \
  -0x1.97dfc994e77aap-1, \
  -0x1.99fe9a973241ep-1, \
  -0x1.99fe9a973241ep-1, \
  -0x1.97dfc994e77aap-1, \
  -0x1.938b320549661p-1, \
  -0x1.8ccf9bc4dd0e7p-1, \
  -0x1.8359e69445b7bp-1, \
  -0x1.76a659f3fa77dp-1, \
  -0x1.65e4c37efca36p-1, \
  -0x1.4fc0ad0d5b772p-1, \
  -0x1.31e63d504db59p-1, \
  -0x1.07c5f850bf06cp-1, \
  -0x1.8d11287aaa09bp-2, \
  -0x1.1fdb7cb3451c8p-3, \
  /* Q = 32 */ \
  -0x1.8b0dd27559608p-3, \
  -0x1.c77a74bd1e552p-2, \
  -0x1.27453d071956ap-1, \
  -0x1.53b85df33e669p-1, \
  -0x1.73ff2d3209badp-1, \
  -0x1.8cb547e5421dbp-1, \
  -0x1.a0395a26c2ecbp-1, \
  -0x1.afeaf3d25a5d2p-1, \
  -0x1.bca6a051c0abep-1, \
  -0x1.c6fe87b425716p-1, \
  -0x1.cf573e29efd99p-1, \
  -0x1.d5f7a24d5f9b5p-1, \
  -0x1.db1221499041ap-1, \
  -0x1.deca59bbbc1c5p-1, \
  -0x1.e1389ca71ed3fp-1, \
  -0x1.e26c17c8c394cp-1, \
  -0x1.e26c17c8c394cp-1, \
  -0x1.e1389ca71ed3fp-1, \
  -0x1.deca59bbbc1c5p-1, \
  -0x1.db1221499041ap-1, \
  -0x1.d5f7a24d5f9b5p-1, \
  -0x1.cf573e29efd99p-1, \
  -0x1.c6fe87b425716p-1, \
  -0x1.bca6a051c0abep-1, \
  -0x1.afeaf3d25a5d2p-1, \
  -0x1.a0395a26c2ecbp-1, \
  -0x1.8cb547e5421dbp-1, \
  -0x1.73ff2d3209badp-1, \
  -0x1.53b85df33e669p-1, \
  -0x1.27453d071956ap-1, \
  -0x1.c77a74bd1e552p-2, \
  -0x1.8b0dd27559608p-3, \
}
