/* Stand-in for the CPU definitions header the IPv4 family includes (see cpu.h here): nothing in it is needed. */
