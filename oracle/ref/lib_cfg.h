/* Stand-in for the library's configuration header: net_util.c needs the file, none of its settings. */
#ifndef NETCSUM_REF_LIB_CFG_H
#define NETCSUM_REF_LIB_CFG_H
#endif
