#FSTBasic MaxPlus
I 0
T 0 1 0 hello -0.5
T 0 2 1 , -1.25
T 1 1 0 , -0.1
T 1 3 2 , -0.7
T 2 2 1
T 2 3 2 world -0.3
T 3 3 2 , -0.2
T 3 4 -1 again -0.9
T 4 1 0 , -0.4
T 3 5 -1
T 5 5 -1 , -0.05
F 3
F 5
